"""Histogram build + approximate quantiles (kernels K3/K6).

Replaces Spark's Greenwald-Khanna `approxQuantile` (rel-err 0.01,
reference stats_generator.py:906-908, quality_checker.py:843-847,
transformers.py:210-215). Algorithm: fused equal-width histogram over all
columns in one kernel (LDS-staged bins on GPU), all-reduced across ranks,
then ADAPTIVE per-quantile bracket refinement passes (LUT-grouped, one
column read serves all of a column's brackets) that run while a bracket's
rank mass exceeds the rel-err tolerance — at production row counts the
2048-bin pass-1 CDF already satisfies Spark's 1% band for smooth columns,
and each further pass narrows a bracket 512x. Only the columns of
unresolved brackets are read again. A bracket whose mass does not split
is cut to the span of its data (a masked min/max); a single value — a
spike — is the answer itself. Columns holding +-inf, and the rare column
that stays unresolved, are sorted.
"""

from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import torch

from anovos_amd.core import dist
from anovos_amd.ops import backend

DEFAULT_BINS = 2048
EXACT_N_THRESHOLD = 250_000  # below this, sort-exact quantiles (GK parity)
# Bound on refinement passes. One pass narrows a bracket 512x (2048x on the
# CPU) and a bracket whose mass does not split is cut to the span of its
# data, so a handful of passes serve any dynamic range; a column that is
# still unresolved after them is sorted.
MAX_REFINE_PASSES = 8
# A bracket narrower than this many ulps of its bounds is not split again:
# its sub-bin bounds (width / 2048 at the finest) would no longer be
# distinct doubles. An f32 ulp is 2^29 f64 ulps, so f32 values still
# separate long before this.
_MIN_SPLIT_ULPS = 4 * 2048
# Bins of one histogram the device quantile query (K3q) holds in LDS
# (QQ_MAX_BINS of ops/hip/anovos_kernels.h)
QQ_MAX_BINS = 4096


def device_quantiles_enabled() -> bool:
    """ANOVOS_DEVICE_QUANTILES=0 turns the device quantile queries (K3q) off:
    pass-1 histograms come back to the host and every bracket is located
    there, as on the CPU (A/B runs, equality tests)."""
    return os.environ.get("ANOVOS_DEVICE_QUANTILES", "1") != "0"


def _on_hip(idf, cols) -> bool:
    t = idf.col(cols[0]).data
    return t.device.type == "cuda" and backend.use_hip(t)


def _pass1_brackets(hist_np, lows, highs, ns, probs):
    """Bracket per (col, prob) from fp64 pass-1 histograms [K, nbins] over
    [lows_i, highs_i] with ns_i non-null values: the bin that contains the
    target rank. Returns (constant, active, brackets, top): {col: value} for
    columns whose range is a single point, the indices of the columns with
    brackets, {(col, prob index): (bl, bh, off, cnt)}, and the set of
    brackets on the last bin. Columns in neither have no values (NaN)."""
    import numpy as np

    nbins = hist_np.shape[1]
    cdf = np.cumsum(hist_np, axis=1)
    # fully vectorized over the (col x prob) grid (the per-pair python loop
    # cost ~5 ms/step at 150x9)
    brackets = {}
    top = set()  # brackets on the last pass-1 bin
    probs_np = np.asarray(probs)
    P = len(probs)
    lows = np.asarray(lows).astype(np.float64)
    valid = (ns > 0) & (lows == lows)
    degenerate = valid & (highs <= lows)
    constant = {int(i): float(lows[i]) for i in np.nonzero(degenerate)[0]}
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
        top = {(int(active[a]), int(j)) for a, j in zip(*np.nonzero(bs == nbins - 1))}
    return constant, active, brackets, top


def _bracket_values(brackets, point, top, highs):
    """{(col, prob index): value} of final brackets (bl, bh, off, cnt), of
    the data values `point` that spike brackets resolved to, and the cap of
    the last pass-1 bin at the column maximum."""
    out = {}
    for k, (bl, bh, off, cnt) in brackets.items():
        if cnt <= 1 or bh <= bl:
            out[k] = bl
        else:
            # interpolate inside the (now tiny) bracket by rank fraction
            frac = min(max(off / max(cnt - 1, 1e-9), 0.0), 1.0) if cnt > 1 else 0.0
            out[k] = bl + frac * (bh - bl)
    for k, v in point.items():
        out[k] = v
    for k in top:
        # the last pass-1 bin's upper bound may round to just above the maximum
        out[k] = min(out[k], float(highs[k[0]]))
    return out


def host_quantile_query(hist, lo, hi, n, probs, rel_err):
    """Quantiles from pass-1 histograms alone, on the host: what
    approx_quantiles returns for brackets that need no refinement. hist is
    [K, nbins] counts, lo / hi / n are per column. Returns fp64 values
    [K, P], bool flags [K, P] (the bracket holds more than rel_err / 2 of
    the rank mass, so approx_quantiles would refine it) and the largest bin
    count [K]. The CPU path, and the reference of the device query (K3q)."""
    import numpy as np

    hist_np = np.asarray(hist).astype(np.float64)
    lows = np.asarray(lo, dtype=np.float64)
    highs = np.asarray(hi, dtype=np.float64)
    ns = np.asarray(n, dtype=np.float64)
    K, P = hist_np.shape[0], len(probs)
    vals = np.full((K, P), float("nan"))
    flags = np.zeros((K, P), dtype=bool)
    constant, active, brackets, top = _pass1_brackets(hist_np, lows, highs, ns, list(probs))
    for i, v in constant.items():
        vals[i, :] = v
    for (i, j), v in _bracket_values(brackets, {}, top, highs).items():
        vals[i, j] = v
    for (i, j), v in brackets.items():
        flags[i, j] = v[3] > rel_err * 0.5 * max(ns[i], 1.0)
    return vals, flags, hist_np.max(axis=1)


def _splittable(bracket):
    import numpy as np

    bl, bh = bracket[0], bracket[1]
    return bh - bl > _MIN_SPLIT_ULPS * float(np.spacing(max(abs(bl), abs(bh))))


def _bracket_extrema(tensors, brackets):
    """(min, max) of the column's values inside [bl, bh) for each bracket
    {(col, prob): (bl, bh, off, cnt)} — a masked reduction over the column,
    used only for brackets whose mass does not split. Returns (inf, -inf)
    when the range does not hold exactly the `cnt` values the histograms
    counted for it, so a caller never resolves to a value of other rows."""
    inf = float("inf")
    uniq = {}
    for k, v in brackets.items():
        uniq.setdefault((k[0], v[0], v[1]), len(uniq))
    dev = tensors[0].device
    red = torch.empty(3, len(uniq), dtype=torch.float64, device=dev)
    red[0], red[1], red[2] = inf, -inf, 0.0
    x64, x64_col = None, None
    for (i, bl, bh), u in sorted(uniq.items()):  # column-major: one fp64 copy per column
        if tensors[i].numel() == 0:
            continue
        if x64_col != i:
            x64, x64_col = tensors[i].to(torch.float64), i
        m = (x64 >= bl) & (x64 < bh)  # NaN compares false
        red[0, u] = torch.where(m, x64, torch.full_like(x64, inf)).min()
        red[1, u] = torch.where(m, x64, torch.full_like(x64, -inf)).max()
        red[2, u] = m.sum()
    dist.all_reduce_(red[0], "min")
    dist.all_reduce_(red[1], "max")
    dist.all_reduce_(red[2], "sum")
    red = red.cpu().tolist()
    out = {}
    for k, v in brackets.items():
        u = uniq[(k[0], v[0], v[1])]
        out[k] = (red[0][u], red[1][u]) if red[2][u] == v[3] else (inf, -inf)
    return out


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


def _exact_integral_quantiles(idf, cols, probs, moments, rel_err=0.0):
    """Exact quantiles for integer-valued columns via one dense
    integer-aligned histogram (bin width exactly 1.0): p <= rel_err ->
    min, p >= 1 - rel_err -> max, else rank = ceil(p*n); value = first
    integer whose CDF reaches the rank — the same query rule as the exact
    sort path (Spark GK returns data elements)."""
    import math as _math

    import numpy as np

    R = {c: int(moments[c].max - moments[c].min) + 1 for c in cols}
    # a column whose dense counts are already cached (an earlier call with
    # other probabilities) is not read again
    use_dev = device_quantiles_enabled() and _on_hip(idf, cols)
    dkey = ("inthist_dev",)
    cold = [c for c in cols if ("inthist",) not in idf.col(c).cache or (use_dev and dkey not in idf.col(c).cache)]
    if cold:
        M = max(R[c] for c in cold)
        lo = torch.tensor([moments[c].min - 0.5 for c in cold], dtype=torch.float64)
        hi = torch.tensor([moments[c].min - 0.5 + M for c in cold], dtype=torch.float64)
        hd = global_histograms([idf.col(c).data for c in cold], lo, hi, M)
        if use_dev:
            # the counts stay on the device as well, with (min, n, R) per column
            meta = torch.tensor([[moments[c].min for c in cold], [float(int(moments[c].n)) for c in cold],
                                 [float(R[c]) for c in cold]], dtype=torch.float64).to(hd.device)
            for i, c in enumerate(cold):
                idf.col(c).cache[dkey] = (hd, meta, i)
    # K3q answers on the device; launched before the counts are fetched
    vals_d = _device_integral_query(idf, cols, probs, rel_err) if use_dev else None
    if cold:
        h = hd.cpu().numpy()
        for i, c in enumerate(cold):
            # the dense per-integer counts serve discrete_modes too — one
            # frame read covers exact quantiles AND exact modes
            idf.col(c).cache[("inthist",)] = (h[i][: R[c]].copy(), float(moments[c].min))
    if vals_d is not None:
        return dict(zip(cols, vals_d.cpu().tolist()))
    out = {}
    for c in cols:
        n = int(moments[c].n)
        counts, cmin = idf.col(c).cache[("inthist",)]
        # every value lies in [min, max], so the counts past R are zero and
        # the truncated CDF gives the same first-reaching index
        cdf = np.cumsum(counts)
        vals = []
        for p in probs:
            if p <= rel_err:
                r = 1
            elif p >= 1 - rel_err:
                r = n
            else:
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
    refine: Optional[int] = None,
    moments: Optional[dict] = None,
    rel_err: float = 1e-2,
) -> Dict[str, List[float]]:
    """Approximate quantiles for each column at the given probabilities.

    Semantics follow Spark approxQuantile (default rel-err 0.01 — the
    reference's summary()/approxQuantile contract): returns a value whose
    rank is within rel_err*n of prob*n. Refinement passes run only for
    brackets that still exceed the rank tolerance (at production row
    counts the 2048-bin pass-1 CDF already satisfies 0.01 for smooth
    columns) and only re-read the columns of those brackets; they repeat
    until every bracket meets the tolerance, at most `refine` times
    (default MAX_REFINE_PASSES). A bracket whose mass will not split — a
    spike — resolves to the data value itself, and a column that cannot
    be resolved this way, or whose min or max is infinite, is sorted.
    """
    import math as _math

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
    # a column that holds +-inf has no finite range to bin over; such
    # columns are rare and are sorted
    inf_cols = [c for c in cols if _math.isinf(moments[c].min) or _math.isinf(moments[c].max)]
    if inf_cols:
        out = _exact_quantiles(idf, inf_cols, probs_l, moments, rel_err=rel_err)
        for c in inf_cols:
            for j, p in enumerate(probs_l):
                idf.col(c).cache[("q", p)] = out[c][j]
        rest = [c for c in cols if c not in set(inf_cols)]
        if rest:
            out.update(approx_quantiles(idf, rest, probs_l, nbins=nbins, refine=refine,
                                        moments=moments, rel_err=rel_err))
        return {c: out[c] for c in cols}
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
        dense = _exact_integral_quantiles(idf, int_cols, probs_l, moments, rel_err=rel_err)
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
    if device_quantiles_enabled() and nbins <= QQ_MAX_BINS and _on_hip(idf, cols):
        # K3q: the histograms stay on the device and are queried there; only
        # the columns with a bracket above the refinement threshold take the
        # host path below
        H, meta = _device_histograms(idf, cols, nbins, moments)
        dv, df, dm = backend.hip_ext().hist_quantile_query(H, meta[0], meta[1], meta[2], probs_l, float(rel_err))
        vals, flagged, maxbin = dv.cpu().tolist(), df.cpu().numpy().any(axis=1), dm.cpu().tolist()
        host_cols = []
        for i, c in enumerate(cols):
            idf.col(c).cache[("hist_maxbin", nbins)] = maxbin[i]
            if flagged[i]:
                host_cols.append(c)
            else:
                for j, p in enumerate(probs_l):
                    idf.col(c).cache[("q", p)] = vals[i][j]
        out = _host_bracket_quantiles(idf, cols, probs_l, nbins, refine, moments, rel_err, only=host_cols) if host_cols else {}
        return {c: out[c] if c in out else vals[i] for i, c in enumerate(cols)}
    return _host_bracket_quantiles(idf, cols, probs_l, nbins, refine, moments, rel_err)


def _device_histograms(idf, cols, nbins, moments):
    """The all-reduced pass-1 histograms of `cols` as one int64
    [ncols, nbins] device tensor, with their fp64 [3, ncols] (lo, hi, n).
    A column's cache holds (matrix, parameters, row) of the call that read
    it; columns not read yet are read here, in one launch."""
    dkey = ("hist_dev", nbins)
    todo = [c for c in cols if dkey not in idf.col(c).cache]
    if todo:
        lo = torch.tensor([moments[c].min for c in todo], dtype=torch.float64)
        hi = torch.tensor([moments[c].max for c in todo], dtype=torch.float64)
        h = global_histograms([idf.col(c).data for c in todo], lo, hi, nbins)
        n = torch.tensor([moments[c].n for c in todo], dtype=torch.float64)
        meta = torch.stack([lo, hi, n]).to(h.device)
        for k, c in enumerate(todo):
            idf.col(c).cache[dkey] = (h, meta, k)
    return _gather_cached_rows([idf.col(c).cache[dkey] for c in cols])


def _gather_cached_rows(entries):
    """(matrix, parameters) of cached (matrix, parameters, row) entries: the
    cached tensors themselves when the entries are all of one call, in its
    order; otherwise the rows are copied together."""
    base, meta, _ = entries[0]
    if all(e[0] is base for e in entries) and [e[2] for e in entries] == list(range(base.shape[0])):
        return base, meta
    if any(e[0].shape[1] != base.shape[1] for e in entries):
        return None, None
    return (torch.stack([e[0][e[2]] for e in entries]),
            torch.stack([e[1][:, e[2]] for e in entries], dim=1).contiguous())


def _device_integral_query(idf, cols, probs, rel_err):
    """Exact quantiles of integral columns from their cached device counts
    (K3q): fp64 [ncols, P] on the device, or None when the cached rows have
    different widths."""
    counts, meta = _gather_cached_rows([idf.col(c).cache[("inthist_dev",)] for c in cols])
    if counts is None:
        return None
    return backend.hip_ext().inthist_quantile_query(counts, meta[0], meta[1], meta[2], list(probs), float(rel_err))


def _is_dense_integral(m) -> bool:
    return bool(m.n > 0 and m.integral and m.min == m.min and 0 < (m.max - m.min) < 4096)


def device_quantile_matrix(idf, cols, probs, nbins: int = DEFAULT_BINS, rel_err: float = 1e-2):
    """approx_quantiles(idf, cols, probs) as an fp64 [ncols, P] tensor that
    never leaves the device, for a consumer that is a kernel: nothing is
    synced. Possible when the device queries are on, every column's
    histogram (or dense integer counts) is cached on the device and no
    column can need refinement: its largest pass-1 bin is within the
    refinement threshold. Returns None otherwise; the caller then takes
    approx_quantiles. When every value is in the ("q", p) caches already
    they are what is returned, as approx_quantiles does."""
    import math as _math

    from anovos_amd.ops import stats as stats_ops

    probs = list(probs)
    if not cols or not probs or not device_quantiles_enabled() or nbins > QQ_MAX_BINS or not _on_hip(idf, cols):
        return None
    moments = stats_ops.frame_moments(idf, cols)
    if all(moments[c].n <= EXACT_N_THRESHOLD for c in cols):
        return None
    if all(all(("q", p) in idf.col(c).cache for p in probs) for c in cols):
        held = [[idf.col(c).cache[("q", p)] for p in probs] for c in cols]
        return torch.tensor(held, dtype=torch.float64).to(idf.col(cols[0]).data.device)
    hist_cols, int_cols = [], []
    for c in cols:
        m, cache = moments[c], idf.col(c).cache
        if _math.isinf(m.min) or _math.isinf(m.max):
            return None
        if _is_dense_integral(m):
            # with every probability cached approx_quantiles no longer takes
            # the column as integral
            if ("inthist_dev",) not in cache or all(("q", p) in cache for p in probs):
                return None
            int_cols.append(c)
        else:
            mb = cache.get(("hist_maxbin", nbins))
            if mb is None or ("hist_dev", nbins) not in cache:
                return None
            # only a column with values over a range has brackets to refine
            ranged = m.n > 0 and m.min == m.min and not m.max <= m.min
            if ranged and mb > rel_err * 0.5 * max(m.n, 1.0):
                return None
            hist_cols.append(c)
    ext = backend.hip_ext()
    parts = []
    if hist_cols:
        H, meta = _device_histograms(idf, hist_cols, nbins, moments)
        parts.append(ext.hist_quantile_query(H, meta[0], meta[1], meta[2], probs, float(rel_err))[0])
    if int_cols:
        v = _device_integral_query(idf, int_cols, probs, rel_err)
        if v is None:
            return None
        parts.append(v)
    out = torch.cat(parts) if len(parts) > 1 else parts[0]
    order = hist_cols + int_cols
    if order != list(cols):
        pos = {c: i for i, c in enumerate(order)}
        out = out.index_select(0, torch.tensor([pos[c] for c in cols], dtype=torch.long).to(out.device))
    return out.contiguous()


def _host_bracket_quantiles(idf, cols, probs, nbins, refine, moments, rel_err, only=None):
    """approx_quantiles for columns with a finite range that are not dense
    integers, brackets located on the host: the CPU path, and on the GPU the
    path of the columns that may need refinement. With `only`, a subset of
    `cols` the device query flagged, just those columns are answered (and
    returned); they keep their positions in `cols`, so the refinement passes
    see the column indices of the whole call."""
    probs_l = probs
    picked = list(cols) if only is None else [c for c in cols if c in set(only)]
    lo = torch.tensor([moments[c].min for c in cols], dtype=torch.float64)
    hi = torch.tensor([moments[c].max for c in cols], dtype=torch.float64)

    # pass-1 histograms are cached per column (range is always the global
    # min/max, so the CDF is reusable across quantile requests)
    key = ("hist", nbins)
    for c in picked:  # read by a device query already: fetch the row
        cache = idf.col(c).cache
        if key not in cache and ("hist_dev", nbins) in cache:
            h, _, row = cache[("hist_dev", nbins)]
            cache[key] = h[row].cpu()
    pos = {c: i for i, c in enumerate(cols)}
    todo = [pos[c] for c in picked if key not in idf.col(c).cache]
    if todo:
        tensors = [idf.col(cols[i]).data for i in todo]
        h = global_histograms(tensors, lo[todo], hi[todo], nbins).cpu()
        for k, i in enumerate(todo):
            idf.col(cols[i]).cache[key] = h[k]
    import numpy as np

    # a column outside `picked` gets an empty row and n = 0: no brackets
    skip = set(cols) - set(picked)
    empty = torch.zeros(nbins, dtype=torch.int64)
    hist_np = torch.stack([empty if c in skip else idf.col(c).cache[key] for c in cols]).numpy().astype(np.float64)
    tensors = [idf.col(c).data for c in cols]

    result = {c: [float("nan")] * len(probs) for c in cols}
    ns = np.array([0.0 if c in skip else moments[c].n for c in cols], dtype=np.float64)
    highs = hi.numpy().astype(np.float64)
    constant, active, brackets, top = _pass1_brackets(hist_np, lo.numpy(), highs, ns, probs)
    for i, v in constant.items():
        result[cols[i]] = [v] * len(probs)
    # adaptive: a bracket is refined while it holds > rel_err/2 of the rank
    # mass (any point of a bracket is within its count of the target rank,
    # so at that size the contract holds with half the tolerance to spare)
    thr = {int(i): rel_err * 0.5 * max(ns[i], 1.0) for i in active}
    point = {}  # (col, prob) -> data value a spike bracket resolved to
    unresolved = set()  # columns that go to the exact sort
    passes = MAX_REFINE_PASSES if refine is None else refine
    over = True  # some bracket is still above the refinement threshold
    for it in range(passes):
        need = {
            k: v for k, v in brackets.items()
            if v[3] > thr[k[0]] and k not in point and k[0] not in unresolved
        }
        over = bool(need)
        need = {k: v for k, v in need.items() if _splittable(v)}
        if not need:
            break
        if it == 0:
            # the pass-1 histogram clamps the column maximum into its last
            # bin; that bin's bracket is half-open, so it ends just above
            # the maximum (children inherit the bound exactly)
            for k in need:
                if k in top:
                    need[k] = (need[k][0], float(np.nextafter(highs[k[0]], np.inf))) + need[k][2:]
        refined = _refine_pass(tensors, cols, need, nbins, lo, hi)
        stuck = {}
        for k, v in refined.items():
            if v[4] != need[k][3]:
                # the sub-histogram does not hold what its parent counted
                # (values within rounding of a bracket bound): the ranks
                # below are no longer known, so the column is sorted
                unresolved.add(k[0])
            elif v[3] == need[k][3]:
                stuck[k] = need[k]  # nothing split off: a spike, or a bracket far wider than its data
            brackets[k] = v[:4]
        stuck = {k: v for k, v in stuck.items() if k[0] not in unresolved}
        if stuck:
            # shrink a bracket whose mass did not split to the span of the
            # values in it; a single value is the answer itself
            for k, (mn, mx) in _bracket_extrema(tensors, stuck).items():
                if not mn <= mx:
                    unresolved.add(k[0])
                elif mn == mx:
                    point[k] = mn
                else:
                    brackets[k] = (mn, float(np.nextafter(mx, np.inf))) + stuck[k][2:]
    # still above the tolerance (out of passes, or at the floating-point
    # resolution of the bounds): a single value resolves to itself,
    # anything else sends the column to the exact sort
    left = {
        k: v for k, v in brackets.items()
        if v[3] > 2.0 * thr[k[0]] and k not in point and k[0] not in unresolved
    } if over else {}
    if left:
        for k, (mn, mx) in _bracket_extrema(tensors, left).items():
            if mn == mx:
                point[k] = mn
            else:
                unresolved.add(k[0])
    for (i, j), v in _bracket_values(brackets, point, top, highs).items():
        result[cols[i]][j] = v
    if unresolved:
        result.update(_exact_quantiles(idf, [cols[i] for i in sorted(unresolved)], probs, moments, rel_err=rel_err))
    for c in picked:
        for j, p in enumerate(probs_l):
            idf.col(c).cache[("q", p)] = result[c][j]
    return {c: result[c] for c in picked}


def _refine_pass(tensors, cols, brackets, nbins, col_lo=None, col_hi=None):
    """One narrowing pass: histogram each active bracket. GPU: ONE grouped
    kernel launch reads every column once and serves all of its brackets
    (512 sub-bins, rank resolution nbins*512 per pass); brackets sit on
    the pass-1 bin grid, so the kernel resolves an element's bracket via
    a pass-1-bin LUT in O(1). CPU: torch loop.

    Returns {key: (lo, hi, off, cnt, total)}: the sub-bin that holds the
    key's rank, and the total of the bracket's sub-histogram, which equals
    the parent's count unless values were lost at a bracket bound."""
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
                # the kernel's rule: pass-1 bin of the bracket's midpoint
                mid = (float(blo[kk]) + float(bhi[kk])) * 0.5
                bin1 = int(min(max((mid - float(p1lo[ci])) * float(p1scale[ci]), 0.0), float(p1bins - 1)))
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
            idx = ((xv - l) * (nbins / (hh - l))).clamp_(0, nbins - 1).long()
            h[kk] = torch.bincount(idx, minlength=nbins)
    dist.all_reduce_(h, "sum")
    import numpy as np

    h_np = h.cpu().numpy().astype(np.float64)
    cdf = np.cumsum(h_np, axis=1)
    totals = cdf[:, -1]
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
        if not bhs[kk] > bls[kk]:
            out[k] = tuple(brackets[k][:4]) + (0.0,)
            continue
        b = int(bs[kk])
        # the last sub-bin ends on the bracket's own bound, so nested
        # brackets tile their parent without a rounding gap at the top
        sub_hi = bhs[kk] if b == nbins - 1 else bls[kk] + (b + 1) * ws[kk]
        out[k] = (float(bls[kk] + b * ws[kk]), float(sub_hi),
                  float(offs[kk] - belows[kk]), float(h_np[urow[kk], b]), float(totals[urow[kk]]))
    return out
