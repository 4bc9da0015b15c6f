"""Histogram build + approximate quantiles (kernels K3/K6).

Replaces Spark's Greenwald-Khanna `approxQuantile` (rel-err 0.01,
reference stats_generator.py:906-908, quality_checker.py:843-847,
transformers.py:210-215). Algorithm: fused equal-width histogram over all
columns in one kernel (LDS-staged bins on GPU), all-reduced across ranks,
then an ADAPTIVE per-quantile bracket refinement pass (LUT-grouped, one
column read serves all of a column's brackets) that only runs while a
bracket's rank mass exceeds the rel-err tolerance — at production row
counts the 2048-bin pass-1 CDF already satisfies Spark's 1% band, and a
second pass reaches rank resolution nbins*512 (≈1e6) when asked for
tighter rel_err.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from anovos_amd.core import dist
from anovos_amd.ops import backend

DEFAULT_BINS = 2048
EXACT_N_THRESHOLD = 250_000  # below this, sort-exact quantiles (GK parity)


def _exact_quantiles(idf, cols, probs, moments, rel_err=1e-4):
    """Exact quantiles by device sort (rocPRIM radix sort via torch.sort);
    Spark GK query semantics (QuantileSummaries.query): p <= relErr ->
    min, p >= 1-relErr -> max, else element at rank ceil(p*n) — the
    float product ceil matters for parity with approxQuantile."""
    import math as _math

    from anovos_amd.core import dist as _dist

    out = {}
    for c in cols:
        t = idf.col(c).data
        x = t[~torch.isnan(t)]
        if _dist.is_dist():
            # tensorized gather (small columns only — EXACT_N_THRESHOLD
            # gates this path); sort on device after the merge
            xs, _ = torch.sort(torch.cat(_dist.all_gather_tensor(x)))
        else:
            xs, _ = torch.sort(x)
        n = xs.numel()
        if n == 0:
            out[c] = [float("nan")] * len(probs)
            continue
        vals = []
        for p in probs:
            if p <= rel_err:
                r = 1
            elif p >= 1 - rel_err:
                r = n
            else:
                r = min(max(int(_math.ceil(p * n)), 1), n)
            vals.append(float(xs[r - 1]))
        out[c] = vals
    return out


def _exact_integral_quantiles(idf, cols, probs, moments):
    """Exact quantiles for integer-valued columns via one dense
    integer-aligned histogram (bin width exactly 1.0): rank = ceil(p*n),
    value = first integer whose CDF reaches the rank — the same rank
    convention as the exact sort path (Spark GK returns data elements)."""
    import math as _math

    import numpy as np

    R = {c: int(moments[c].max - moments[c].min) + 1 for c in cols}
    # a column whose dense counts are already cached (an earlier call with
    # other probabilities) is not read again
    cold = [c for c in cols if ("inthist",) not in idf.col(c).cache]
    if cold:
        M = max(R[c] for c in cold)
        lo = torch.tensor([moments[c].min - 0.5 for c in cold], dtype=torch.float64)
        hi = torch.tensor([moments[c].min - 0.5 + M for c in cold], dtype=torch.float64)
        h = global_histograms([idf.col(c).data for c in cold], lo, hi, M).cpu().numpy()
        for i, c in enumerate(cold):
            # the dense per-integer counts serve discrete_modes too — one
            # frame read covers exact quantiles AND exact modes
            idf.col(c).cache[("inthist",)] = (h[i][: R[c]].copy(), float(moments[c].min))
    out = {}
    for c in cols:
        n = int(moments[c].n)
        counts, cmin = idf.col(c).cache[("inthist",)]
        # every value lies in [min, max], so the counts past R are zero and
        # the truncated CDF gives the same first-reaching index
        cdf = np.cumsum(counts)
        vals = []
        for p in probs:
            r = min(max(int(_math.ceil(p * n)), 1), n)
            b = int(np.searchsorted(cdf, r, side="left"))
            vals.append(float(cmin + min(b, R[c] - 1)))
        out[c] = vals
    return out


def column_histograms(
    tensors: Sequence[torch.Tensor],
    lo: torch.Tensor,
    hi: torch.Tensor,
    nbins: int = DEFAULT_BINS,
) -> torch.Tensor:
    """Per-column equal-width histograms over [lo_i, hi_i].

    Values outside the range are clamped into the edge bins (the range is
    normally the column's global min/max so nothing clips). NaN skipped.
    Returns int64 [ncols, nbins] LOCAL counts on the device.
    """
    ncols = len(tensors)
    dev = tensors[0].device if ncols else torch.device("cpu")
    if ncols and dev.type == "cuda" and backend.use_hip(tensors[0]):
        ext = backend.hip_ext()
        return ext.column_histograms([t.contiguous() for t in tensors], lo.to(dev), hi.to(dev), nbins)
    out = torch.zeros(ncols, nbins, dtype=torch.int64, device=dev)
    for i, t in enumerate(tensors):
        x = t[~torch.isnan(t)].to(torch.float64)
        l, h = float(lo[i]), float(hi[i])
        if x.numel() == 0 or not (h > l):
            # no usable range (constant column, or hi < lo): every
            # non-null value counts in bin 0, as in the kernel
            out[i, 0] = x.numel()
            continue
        # clamp in floating point first, as the kernel does: .long() of
        # +-inf is not defined (it put +inf into bin 0)
        idx = ((x - l) * (nbins / (h - l))).clamp_(0, nbins - 1).long()
        out[i] = torch.bincount(idx, minlength=nbins)
    return out


def global_histograms(tensors, lo, hi, nbins=DEFAULT_BINS) -> torch.Tensor:
    h = column_histograms(tensors, lo, hi, nbins)
    dist.all_reduce_(h, "sum")
    return h


def approx_quantiles(
    idf,
    cols: List[str],
    probs: Sequence[float],
    nbins: int = DEFAULT_BINS,
    refine: int = 1,
    moments: Optional[dict] = None,
    rel_err: float = 1e-2,
) -> Dict[str, List[float]]:
    """Approximate quantiles for each column at the given probabilities.

    Semantics follow Spark approxQuantile (default rel-err 0.01 — the
    reference's summary()/approxQuantile contract): returns a value whose
    rank is within rel_err*n of prob*n. The adaptive refinement pass only
    runs for brackets whose pass-1 bin still exceeds the rank tolerance
    (at production row counts the 2048-bin pass-1 CDF already satisfies
    0.01); pass a smaller rel_err for tighter interpolation.
    """
    from anovos_amd.ops import stats as stats_ops

    if moments is None:
        moments = stats_ops.frame_moments(idf, cols)
    # Exact path for small columns: Spark's GK sketch returns actual data
    # elements (rank = ceil(p*n)); reference tests assert 4-decimal values,
    # so below this size we sort-and-index instead of sketching.
    if all(moments[c].n <= EXACT_N_THRESHOLD for c in cols):
        return _exact_quantiles(idf, cols, probs, moments, rel_err=rel_err)
    # value cache keyed per (col, prob): sections share quantile work
    # (percentiles computes 1..99%; outlier/imputation reuse 5/50/95%)
    probs_l = list(probs)
    if all(all(("q", p) in idf.col(c).cache for p in probs_l) for c in cols):
        return {c: [idf.col(c).cache[("q", p)] for p in probs_l] for c in cols}
    dev = idf.device
    # integral columns with bounded range: EXACT quantiles from one
    # dense integer-aligned histogram (the generic 2048-bin pass-1 puts
    # each integer in a spike bin that always exceeds the rank tolerance
    # and forces a refinement read; this path is one read, exact, and
    # returns actual data elements like Spark's GK sketch)
    int_cols = [
        c for c in cols
        if moments[c].n > 0 and moments[c].integral
        and moments[c].min == moments[c].min
        and 0 < (moments[c].max - moments[c].min) < 4096
        and any(("q", p) not in idf.col(c).cache for p in probs_l)
    ]
    if int_cols:
        dense = _exact_integral_quantiles(idf, int_cols, probs_l, moments)
        for c in int_cols:
            for j, p in enumerate(probs_l):
                idf.col(c).cache[("q", p)] = dense[c][j]
        rest = [c for c in cols if c not in set(int_cols)]
        if not rest:
            return {c: [idf.col(c).cache[("q", p)] for p in probs_l] for c in cols}
        out = approx_quantiles(idf, rest, probs_l, nbins=nbins, refine=refine,
                               moments=moments, rel_err=rel_err)
        out.update(dense)
        return {c: out[c] for c in cols}
    lo = torch.tensor([moments[c].min for c in cols], dtype=torch.float64)
    hi = torch.tensor([moments[c].max for c in cols], dtype=torch.float64)
    probs = list(probs)

    # pass-1 histograms are cached per column (range is always the global
    # min/max, so the CDF is reusable across quantile requests)
    key = ("hist", nbins)
    todo = [i for i, c in enumerate(cols) if key not in idf.col(c).cache]
    if todo:
        tensors = [idf.col(cols[i]).data for i in todo]
        h = global_histograms(tensors, lo[todo], hi[todo], nbins).cpu()
        for k, i in enumerate(todo):
            idf.col(cols[i]).cache[key] = h[k]
    import numpy as np

    hist_np = torch.stack([idf.col(c).cache[key] for c in cols]).numpy().astype(np.float64)
    cdf = np.cumsum(hist_np, axis=1)
    tensors = [idf.col(c).data for c in cols]

    result = {c: [float("nan")] * len(probs) for c in cols}
    # bracket per (col, prob): bin containing target rank — fully
    # vectorized over the (col x prob) grid (the per-pair python loop
    # cost ~5 ms/step at 150x9)
    brackets = {}
    probs_np = np.asarray(probs)
    K, P = len(cols), len(probs)
    ns = np.array([moments[c].n for c in cols], dtype=np.float64)
    lows = lo.numpy().astype(np.float64)
    highs = hi.numpy().astype(np.float64)
    valid = (ns > 0) & (lows == lows)
    degenerate = valid & (highs <= lows)
    for i in np.nonzero(degenerate)[0]:
        result[cols[i]] = [float(lows[i])] * P
    active = np.nonzero(valid & ~degenerate)[0]
    if active.size:
        w = (highs[active] - lows[active]) / nbins  # [A]
        targets = probs_np[None, :] * (ns[active, None] - 1)  # [A,P]
        # vectorized per-row searchsorted: count of cdf entries < target
        cdf_a = cdf[active]  # [A,nbins]
        bs = np.minimum((cdf_a[:, :, None] < (targets + 0.5)[:, None, :]).sum(axis=1), nbins - 1)  # [A,P]
        rows = np.arange(active.size)[:, None]
        belows = np.where(bs > 0, cdf_a[rows, np.maximum(bs - 1, 0)], 0.0)
        cnts = hist_np[active][rows, bs]
        for a, i in enumerate(active):
            l = lows[i]
            wa = w[a]
            for j in range(P):
                b = int(bs[a, j])
                brackets[(int(i), j)] = (l + b * wa, l + (b + 1) * wa, float(targets[a, j] - belows[a, j]), float(cnts[a, j]))
    for _ in range(refine):
        # adaptive: only brackets whose bin still holds > rel_err/2 of the
        # rank mass need another pass (Spark guarantees 1% rank error;
        # within-bin interpolation already bounds ours by bin_count/n)
        need = {
            k: v
            for k, v in brackets.items()
            if v[3] > rel_err * 0.5 * max(moments[cols[k[0]]].n, 1)
        }
        if not need:
            break
        refined = _refine_pass(tensors, cols, need, nbins, lo, hi)
        brackets.update(refined)
    for (i, j), (bl, bh, off, cnt) in brackets.items():
        c = cols[i]
        if cnt <= 1 or bh - bl < 1e-12 * max(1.0, abs(bl)):
            result[c][j] = bl
        else:
            # interpolate inside the (now tiny) bracket by rank fraction
            frac = min(max(off / max(cnt - 1, 1e-9), 0.0), 1.0) if cnt > 1 else 0.0
            result[c][j] = bl + frac * (bh - bl)
    for c in cols:
        for j, p in enumerate(probs_l):
            idf.col(c).cache[("q", p)] = result[c][j]
    return result


def _refine_pass(tensors, cols, brackets, nbins, col_lo=None, col_hi=None):
    """One narrowing pass: histogram each active bracket. GPU: ONE grouped
    kernel launch reads every column once and serves all of its brackets
    (512 sub-bins, rank resolution nbins*512 per pass); brackets sit on
    the pass-1 bin grid, so the kernel resolves an element's bracket via
    a pass-1-bin LUT in O(1). CPU: torch loop."""
    if not brackets:
        return brackets
    all_keys = sorted(brackets.keys())  # sorted by (col, prob) — grouped kernel needs col-major
    # dedupe identical (col, range) brackets: several probs often land in
    # the SAME pass-1 bin (heavy-duplicate data) and the kernel's
    # bin→bracket LUT holds one entry per bin — the shared histogram
    # serves every prob that maps to it
    uniq = {}
    key_to_uniq = {}
    for k in all_keys:
        u = (k[0], brackets[k][0], brackets[k][1])
        if u not in uniq:
            uniq[u] = len(uniq)
        key_to_uniq[k] = uniq[u]
    keys = [None] * len(uniq)
    for k in all_keys:
        if keys[key_to_uniq[k]] is None:
            keys[key_to_uniq[k]] = k
    dev = tensors[0].device
    blo = torch.tensor([brackets[k][0] for k in keys], dtype=torch.float64)
    bhi = torch.tensor([brackets[k][1] for k in keys], dtype=torch.float64)
    colidx = torch.tensor([k[0] for k in keys], dtype=torch.int64)
    if dev.type == "cuda" and backend.use_hip(tensors[0]):
        ext = backend.hip_ext()
        p1bins = nbins
        degenerate = col_lo is None
        if degenerate:  # treat each bracket as its own grid
            col_lo = blo.clone()
            col_hi = bhi.clone()
        p1lo = col_lo.to(torch.float64)
        rng = (col_hi.to(torch.float64) - p1lo).clamp(min=1e-300)
        p1scale = float(p1bins) / rng
        nbins = 512  # grouped kernel's fixed sub-bin count
        # Partition brackets into launch groups honoring the kernel's two
        # structural limits: <= 16 brackets per column per
        # launch, and no two brackets of a column in the SAME pass-1 bin
        # (the LDS bin->bracket LUT holds one entry per bin — a collision
        # silently zeroes the losing bracket). Spiky distributions with
        # many refinement brackets go through extra launches instead of
        # crashing / silently degrading.
        groups, seen = [], []
        for kk, k in enumerate(keys):
            ci = k[0]
            if degenerate:
                bin1 = 0
            else:
                bin1 = int((float(blo[kk]) - float(p1lo[ci])) * float(p1scale[ci]) + 1e-6)
            placed = False
            for gi, g in enumerate(groups):
                bins_here = seen[gi].setdefault(ci, set())
                if len(bins_here) < 16 and bin1 not in bins_here:
                    g.append(kk)
                    bins_here.add(bin1)
                    placed = True
                    break
            if not placed:
                groups.append([kk])
                seen.append({ci: {bin1}})
        tens_c = [t.contiguous() for t in tensors]
        # the grouped kernel launches one dtype at a time — split each
        # launch group by column dtype (mixed f32/f64 frames arise when
        # the pipeline runs HBM-resident without a parquet round-trip)
        split_groups = []
        for g in groups:
            f32 = [kk for kk in g if tens_c[keys[kk][0]].dtype == torch.float32]
            f64 = [kk for kk in g if tens_c[keys[kk][0]].dtype != torch.float32]
            if f32:
                split_groups.append(f32)
            if f64:
                split_groups.append(f64)
        h = torch.zeros(len(keys), nbins, dtype=torch.int64, device=dev)
        for g in split_groups:
            gi_t = torch.tensor(g, dtype=torch.long)
            hg = ext.bracket_histograms_grouped(tens_c, colidx[gi_t], blo[gi_t], bhi[gi_t],
                                                p1lo, p1scale, p1bins)
            h[gi_t] = hg
    else:
        h = torch.zeros(len(keys), nbins, dtype=torch.int64, device=dev)
        for kk, (i, j) in enumerate(keys):
            t = tensors[i]
            x = t[~torch.isnan(t)].to(torch.float64)
            l, hh = float(blo[kk]), float(bhi[kk])
            if hh <= l:
                continue
            m = (x >= l) & (x < hh)
            xv = x[m]
            if xv.numel() == 0:
                continue
            idx = ((xv - l) * (nbins / (hh - l))).long().clamp_(0, nbins - 1)
            h[kk] = torch.bincount(idx, minlength=nbins)
    dist.all_reduce_(h, "sum")
    import numpy as np

    h_np = h.cpu().numpy().astype(np.float64)
    cdf = np.cumsum(h_np, axis=1)
    # resolve EVERY original (col, prob) key against its (possibly
    # shared) bracket histogram — off differs per prob even when the
    # range is shared
    urow = np.array([key_to_uniq[k] for k in all_keys])
    bls = np.array([brackets[k][0] for k in all_keys])
    bhs = np.array([brackets[k][1] for k in all_keys])
    offs = np.array([brackets[k][2] for k in all_keys])
    bs = np.minimum((cdf[urow] < (offs + 0.5)[:, None]).sum(axis=1), nbins - 1)
    rows = np.arange(len(all_keys))
    belows = np.where(bs > 0, cdf[urow, np.maximum(bs - 1, 0)], 0.0)
    ws = (bhs - bls) / nbins
    out = {}
    for kk, k in enumerate(all_keys):
        if bhs[kk] <= bls[kk]:
            out[k] = brackets[k]
            continue
        b = int(bs[kk])
        out[k] = (bls[kk] + b * ws[kk], bls[kk] + (b + 1) * ws[kk],
                  float(offs[kk] - belows[kk]), float(h_np[urow[kk], b]))
    return out
