"""Point-in-polygon membership of (lat, lon) column pairs (kernel K33): one
f32 column per pair, NaN where lat or lon is null, else 1.0 inside any ring,
else 0.0. Inside a ring is odd crossing parity under the rule of
``geo_utils.point_in_polygon``:

    straddles = (py > y) != (qy > y)
    crosses   = straddles and x < px + (y - py) * (qx - px) / (qy - py)

in fp64 with x = lon, y = lat, parity per ring, OR over rings.

- HIP path (ops/hip/polygon_raycast.hip): a row tests only the edges of its
  own latitude band; ``edge_table`` builds the band index once per call for
  all pairs. f32 and f64 columns are read as they are.
- CPU backend: the torch expression of geo_utils in row slabs of a bounded
  scratch.

Both give the same values; neither allocates rows x edges.
"""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from anovos_amd.ops import backend

# PIP_RECORD_BYTES and PIP_LDS_BYTES of ops/hip/anovos_kernels.h: the image a
# block can stage in LDS
PIP_RECORD_BYTES = 48
PIP_LDS_BYTES = 40 * 1024
PIP_AUTO_MAX_BANDS = 16384
# fp64 scratch of one slab of the library path (about six [rows, E] temporaries)
PIP_SLAB_BYTES = 64 << 20


def auto_bands(n_edges: int) -> int:
    """Bands edge_table starts from for E edges (docs/KERNELS.md, K33, has the
    sweep): a row's cost is the length of its band's list, which stops
    falling near 2 E bands for a convex outline."""
    return int(min(max(4 * n_edges, 1), PIP_AUTO_MAX_BANDS))


def fits_lds(n_records: int, bands: int) -> bool:
    return PIP_RECORD_BYTES * n_records + 4 * (bands + 4) <= PIP_LDS_BYTES


def band_index(y, ymin: float, scale: float, bands: int):
    """band(y) for ymin <= y <= ymax, the expression of the kernel: subtract,
    multiply, floor, clamp - each monotone, none contracted."""
    f = np.floor((np.asarray(y, dtype=np.float64) - ymin) * scale)
    return np.where(f < bands - 1, f, bands - 1).astype(np.int64)


def edge_table(rings: Sequence, bands: Optional[int] = None):
    """(edges, band_off, band_edges, meta) of a ring set, numpy.

    edges fp64 [E, 5] = (px, py, qx, qy, ring) in (lon, lat) order, every ring
    closed on itself, horizontal edges dropped (they never straddle; this
    covers a repeated closing vertex). meta = (ymin, ymax, scale) over the
    edges, scale = B / (ymax - ymin). band_edges[band_off[b] : band_off[b + 1]]
    are the edges that overlap band b, in ring order: an edge is filed under
    band(min(py, qy)) .. band(max(py, qy)), so every edge that straddles y is
    in the list of band(y)."""
    recs = []
    for rid, ring in enumerate(rings):
        v = np.asarray(ring, dtype=np.float64)[:, :2]
        q = np.roll(v, -1, axis=0)
        keep = v[:, 1] != q[:, 1]
        recs.append(np.column_stack([v[keep], q[keep], np.full(int(keep.sum()), float(rid))]))
    edges = np.concatenate(recs) if recs else np.zeros((0, 5))
    E = len(edges)
    if E == 0:  # nothing straddles anything: every row is outside
        return edges, np.zeros(2, np.int32), np.zeros(0, np.int32), np.array([np.inf, -np.inf, 0.0])
    lo, hi = np.minimum(edges[:, 1], edges[:, 3]), np.maximum(edges[:, 1], edges[:, 3])
    ymin, ymax = float(lo.min()), float(hi.max())

    def filed(B):
        scale = B / (ymax - ymin)
        if not (np.isfinite(scale) and scale > 0):
            raise ValueError("edge_table: latitude extent of the rings is not finite")
        b0 = band_index(lo, ymin, scale, B)
        return scale, b0, band_index(hi, ymin, scale, B) - b0 + 1

    B = int(bands) if bands else auto_bands(E)
    scale, b0, copies = filed(B)
    if not bands:
        # long edges are copied into every band they cross: stop where the
        # copies outgrow the bands
        while B > 1 and int(copies.sum()) > 16 * E + 4 * B:
            B //= 2
            scale, b0, copies = filed(B)
        # an image that fits LDS is worth lists up to twice as long
        Bl = B
        while not fits_lds(int(copies.sum()), Bl) and Bl // 2 >= E:
            Bl //= 2
            scale, b0, copies = filed(Bl)
        if fits_lds(int(copies.sum()), Bl):
            B = Bl
        else:
            scale, b0, copies = filed(B)
    eid = np.repeat(np.arange(E), copies)
    band = np.repeat(b0, copies) + (np.arange(len(eid)) - np.repeat(np.cumsum(copies) - copies, copies))
    # by band, then by edge: edges are numbered ring by ring
    order = np.lexsort((eid, band))
    band_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.bincount(band, minlength=B), out=band_off[1:])
    return edges, band_off.astype(np.int32), eid[order].astype(np.int32), np.array([ymin, ymax, scale])


def _column(src, c) -> torch.Tensor:
    """A lat / lon column: a tensor as it is, a frame column by name.
    Categorical and integer columns become fp64 through geospatial._num."""
    if torch.is_tensor(c):
        t = c
    else:
        col = src.col(c)
        if col.kind == "categorical" or not col.data.is_floating_point():
            from anovos_amd.data_transformer.geospatial import _num

            return _num(src, c)
        t = col.data
    return t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float64)


def points_in_polygons(idf_or_tensors, pairs: Sequence, rings: Sequence, slab_rows: Optional[int] = None,
                       bands: Optional[int] = None) -> List[torch.Tensor]:
    """One f32 tensor per (lat, lon) pair. `pairs` names columns of the frame
    `idf_or_tensors`, or holds tensors (the first argument is then unused).
    `rings` are sequences of (lon, lat) vertices. `slab_rows` bounds the rows
    of one slab of the library path, `bands` overrides the band count."""
    cols = [(_column(idf_or_tensors, la), _column(idf_or_tensors, lo)) for la, lo in pairs]
    if not cols:
        return []
    if cols[0][0].is_cuda and backend.use_hip(cols[0][0]):
        lats, lons = [], []
        for la, lo in cols:
            if la.dtype != lo.dtype:
                la, lo = la.to(torch.float64), lo.to(torch.float64)
            lats.append(la.contiguous())
            lons.append(lo.contiguous())
        edges, band_off, band_edges, meta = edge_table(rings, bands)
        return backend.hip_ext().points_in_polygons(
            lats, lons, torch.from_numpy(edges), torch.from_numpy(band_off), torch.from_numpy(band_edges),
            torch.from_numpy(meta), None)
    from anovos_amd.data_transformer import geo_utils as gu

    n_edges = max(1, sum(len(r) for r in rings))
    slab = int(slab_rows or max(1, PIP_SLAB_BYTES // (48 * n_edges)))
    outs = []
    for la, lo in cols:
        n = int(la.shape[0])
        out = torch.empty(n, dtype=torch.float32, device=la.device)
        for r0 in range(0, n, slab):
            y, x = la[r0:r0 + slab].to(torch.float64), lo[r0:r0 + slab].to(torch.float64)
            v = gu.point_in_polygons(y, x, rings).to(torch.float32)
            out[r0:r0 + slab] = torch.where(torch.isnan(y) | torch.isnan(x), torch.full_like(v, float("nan")), v)
        outs.append(out)
    return outs
