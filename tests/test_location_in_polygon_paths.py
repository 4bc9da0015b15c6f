"""ops.polygon and the geospatial functions on it: the slabbed library path
against geo_utils, the band index against its correctness condition, and on
the GPU location_in_polygon / location_in_country("exact") against the numpy
reference of tests/test_polygon_raycast_kernel.py, with the memory the call
takes."""

import json

import numpy as np
import pytest
import torch

from anovos_amd.core.frame import AnovosFrame, Column
from anovos_amd.data_transformer import geo_utils as gu
from anovos_amd.data_transformer import geospatial as geo
from anovos_amd.ops.polygon import band_index, edge_table, points_in_polygons
from test_polygon_raycast_kernel import RING_SETS, points, reference

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

RINGS = RING_SETS["overlap"] + RING_SETS["comb"]
MULTIPOLYGON = {"type": "MultiPolygon", "coordinates": [[[list(v) for v in r]] for r in RINGS]}


def same(got, want):
    return bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def test_slabbed_library_path_equals_geo_utils():
    lat, lon = (torch.from_numpy(a) for a in points(RINGS, 1000, 5))
    (got,) = points_in_polygons(None, [(lat, lon)], RINGS, slab_rows=96)
    keep = ~(torch.isnan(lat) | torch.isnan(lon))
    assert got.dtype == torch.float32 and torch.isnan(got[~keep]).all()
    assert torch.equal(got[keep], gu.point_in_polygons(lat, lon, RINGS)[keep].float())
    assert same(got.numpy(), reference(lat.numpy(), lon.numpy(), RINGS))


@pytest.mark.parametrize("bands", [1, 2, 37, None])
@pytest.mark.parametrize("name", list(RING_SETS))
def test_edge_table_lists_every_straddling_edge(name, bands):
    """For every point and every edge that straddles its latitude, the edge is in the list of
    the point's band; lists are in ring order and hold no horizontal edge."""
    edges, off, be, (ymin, ymax, scale) = edge_table(RING_SETS[name], bands)
    B = len(off) - 1
    assert off[0] == 0 and off[-1] == len(be) and (np.diff(off) >= 0).all()
    assert (edges[:, 1] != edges[:, 3]).all()
    listed = np.zeros((B, len(edges)), dtype=bool)
    for b in range(B):
        mine = be[off[b]:off[b + 1]]
        listed[b, mine] = True
        assert (np.diff(edges[mine, 4]) >= 0).all()
    lat, _ = points(RING_SETS[name], 600, B)
    lat = lat[(lat >= ymin) & (lat <= ymax)]
    y = lat[:, None]
    straddles = (edges[:, 1] > y) != (edges[:, 3] > y)
    assert straddles.any() and not (straddles & ~listed[band_index(lat, ymin, scale, B)]).any()


def _frame(n, dev, seed):
    """lat1 / lon1 f32, lat2 / lon2 f64, with nulls; and the columns as numpy."""
    la, lo = points(RINGS, n, 3, seed=seed)
    with np.errstate(over="ignore"):  # 1e300 is inf in f32
        cols = {"lat1": la.astype(np.float32), "lon1": lo.astype(np.float32), "lat2": la[::-1].copy(),
                "lon2": lo[::-1].copy()}
    frame = AnovosFrame({k: Column(k, "float" if v.dtype == np.float32 else "double", torch.from_numpy(v).to(dev))
                         for k, v in cols.items()}, dev)
    return frame, cols


@needs_gpu
@pytest.mark.gpu
def test_gpu_functions_equal_reference(ctx, tmp_path):
    idf, cols = _frame(3000, "cuda", 2)
    odf = geo.location_in_polygon(idf, ["lat1", "lat2"], ["lon1", "lon2"], MULTIPOLYGON)
    path = tmp_path / "country.json"
    path.write_text(json.dumps({"type": "FeatureCollection", "features": [
        {"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [[list(v) for v in r]]}} for r in RINGS]}))
    cdf = geo.location_in_country(ctx, idf, ["lat1", "lat2"], ["lon1", "lon2"], "Atlantis", str(path),
                                  method_type="exact", result_prefix=["a", "b"], output_mode="replace")
    assert cdf.columns == ["a_in_atlantis", "b_in_atlantis"]
    for k, (new, other) in enumerate([("lat1_lon1_in_polygon", "a_in_atlantis"), ("lat2_lon2_in_polygon", "b_in_atlantis")]):
        want = reference(cols[f"lat{k + 1}"], cols[f"lon{k + 1}"], RINGS)
        for frame, name in ((odf, new), (cdf, other)):
            c = frame.col(name)
            assert c.dtype == "int" and c.data.dtype == torch.float32
            assert same(c.data.cpu().numpy(), want)


@needs_gpu
@pytest.mark.gpu
def test_gpu_memory_is_linear_in_rows():
    """1M rows against a 2 000-edge ring: at most 64 B per row beyond the table (two f64
    copies and the f32 output are 20 B); one [rows, edges] fp64 matrix would be 16 GB."""
    n = 1_000_000
    ring = RING_SETS["gon"][0][:2000]
    g = torch.Generator(device="cuda").manual_seed(5)
    lat = 50 + 6 * (torch.rand(n, device="cuda", generator=g) - 0.5)
    lon = 10 + 9 * (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) - 0.5)
    idf = AnovosFrame({"lat": Column("lat", "float", lat), "lon": Column("lon", "double", lon)}, "cuda")
    edges, off, be, _ = edge_table([ring])
    # the image, the uploaded edge list and index, and 512-byte rounding of a dozen small uploads
    table_bytes = 48 * len(be) + 4 * len(off) + edges.nbytes + off.nbytes + be.nbytes + 16 * 512
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    odf = geo.location_in_polygon(idf, ["lat"], ["lon"], [ring])
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} B for {n} rows")
    assert rise < 64 * n + table_bytes
    got = odf.col("lat_lon_in_polygon").data[:2000].cpu().numpy()
    assert same(got, reference(lat[:2000].cpu().numpy(), lon[:2000].cpu().numpy(), [ring]))
