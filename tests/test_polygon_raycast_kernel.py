"""The point-in-polygon kernel K33 (ops/hip/polygon_raycast.hip, whose header
states the operation) against a plain numpy fp64 evaluation of the crossing
rule, ring by ring. The arithmetic is specified to be the same, so the whole
sentinel-filled output buffer must have the expectation's bits: no tolerance,
nothing left out. ANOVOS_PIP_BLOCKS forces the grid, so small inputs reach
partial tiles, several tiles per block and blocks without work."""

import functools

import numpy as np
import pytest
import torch

from anovos_amd.ops.polygon import edge_table

pytestmark = [pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"), pytest.mark.gpu]

DEV = "cuda"


def _gon(m):
    rng = np.random.default_rng(33)
    a = np.sort(rng.uniform(0, 2 * np.pi, m))
    r = 1 + 0.2 * rng.random(m)
    return [np.column_stack([10 + 3 * r * np.cos(a), 50 + 2 * r * np.sin(a)]).tolist()]


RING_SETS = {
    "triangle": [[(0, 0), (4, 1), (1.5, 3)]],
    # closing vertex repeated: a zero-length edge and two horizontal ones
    "square": [[(0, 0), (1, 0), (1, 1), (0, 1), (0, 0)]],
    # a ray at y = 2 crosses 8 edges
    "comb": [[(0, 0), (7, 0), (7, 3), (6, 3), (6, 1), (5, 1), (5, 3), (4, 3), (4, 1), (3, 1), (3, 3), (2, 3),
              (2, 1), (1, 1), (1, 3), (0, 3)]],
    # the overlap is inside: OR of the rings, not one parity over all edges
    "overlap": [[(0, 0), (2, 0), (2, 2), (0, 2)], [(1, 1), (3, 1), (3, 3), (1, 3)]],
    "disjoint": [[(0, 0), (1, 0.2), (0.5, 1)], [(3, 3), (4, 3), (4, 4.5), (3, 4)]],
    # 5 000 edges: 240 kB of records, beyond the LDS budget
    "gon": _gon(5000),
}


def reference(lat, lon, rings):
    """1 / 0 / NaN as f32: the crossing rule in fp64, parity per ring, OR over rings."""
    x, y = lon.astype(np.float64)[:, None], lat.astype(np.float64)[:, None]
    inside = np.zeros(len(lat), dtype=bool)
    for ring in rings:
        px, py = np.asarray(ring, dtype=np.float64).T
        qx, qy = np.roll(px, -1), np.roll(py, -1)
        straddles = (py > y) != (qy > y)
        with np.errstate(all="ignore"):
            crosses = straddles & (x < px + (y - py) * (qx - px) / np.where(straddles, qy - py, 1.0))
        inside |= crosses.sum(axis=1) % 2 == 1
    out = inside.astype(np.float32)
    out[np.isnan(lat) | np.isnan(lon)] = np.nan
    return out


def points(rings, n, bands, seed=0):
    """(lat, lon) fp64: NaN rows, points far outside, then every vertex and points at ymin,
    ymax and on and next to every band boundary (a seeded subset if they outnumber n / 2),
    the rest uniform over 1.5 x the bounding box."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([np.asarray(r, dtype=np.float64) for r in rings])
    (x0, y0), (x1, y1) = v.min(axis=0), v.max(axis=0)
    cy = y0 + np.arange(bands + 1) * ((y1 - y0) / bands)
    cy = np.concatenate([cy, np.nextafter(cy, -np.inf), np.nextafter(cy, np.inf)])
    sx = np.concatenate([v[:, 0], rng.uniform(x0 - 0.5, x1 + 0.5, len(cy))])
    sy = np.concatenate([v[:, 1], cy])
    pick = rng.permutation(len(sx))[:max(0, n // 2 - 7)]
    nan = np.nan
    sx = np.concatenate([[nan, 1.0, nan, 1e300, -1e300, x0, x1], sx[pick]])[:n]
    sy = np.concatenate([[1.0, nan, nan, y0, y1, 1e300, -np.inf], sy[pick]])[:n]
    w, h = 1.5 * (x1 - x0), 1.5 * (y1 - y0)
    lon = np.concatenate([sx, rng.uniform((x0 + x1 - w) / 2, (x0 + x1 + w) / 2, n - len(sx))])
    lat = np.concatenate([sy, rng.uniform((y0 + y1 - h) / 2, (y0 + y1 + h) / 2, n - len(sy))])
    return lat, lon


@functools.lru_cache(maxsize=None)
def case(name, n, bands, f32):
    """Two pairs (the second is the first reversed) in the column dtype, and their
    expectation: the reference sees the values the columns hold."""
    lat, lon = points(RING_SETS[name], n, bands)
    dt = np.float32 if f32 else np.float64
    with np.errstate(over="ignore"):  # 1e300 is inf in f32
        pairs = [(lat.astype(dt), lon.astype(dt)), (lat[::-1].astype(dt), lon[::-1].astype(dt))]
    return pairs, [reference(la, lo, RING_SETS[name]) for la, lo in pairs]


def run(ext, pairs, table, bands=0, mode="auto"):
    """The sentinel buffer after the call, outs[p] = buf[p, 3 : 3 + n_p]."""
    nmax = max(len(la) for la, _ in pairs)
    buf = torch.full((len(pairs), nmax + 5), -7.0, dtype=torch.float32, device=DEV)
    dev = lambda a: torch.as_tensor(a.copy()).to(DEV)
    ext.points_in_polygons([dev(la) for la, _ in pairs], [dev(lo) for _, lo in pairs],
                           *[torch.from_numpy(t) for t in table],
                           [buf[p, 3:3 + len(la)] for p, (la, _) in enumerate(pairs)], bands=bands, table=mode)
    return buf.cpu().numpy()


def expected(pairs, refs):
    want = np.full((len(pairs), max(len(r) for r in refs) + 5), -7.0, dtype=np.float32)
    for p, r in enumerate(refs):
        want[p, 3:3 + len(r)] = r
    return want


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    return backend.require_hip()


# (n, ANOVOS_PIP_BLOCKS, f32 columns): partial and several 1024-row tiles, idle blocks
ROWS = [(1, 1, False), (63, 3, True), (64, 1, False), (65, 3, True), (257, 3, False), (1027, 1, True),
        (1027, 3, False)]
TABLES = [(name, mode) for name in RING_SETS for mode in ("lds", "global") if (name, mode) != ("gon", "lds")]


@pytest.mark.parametrize("rows", ROWS, ids=lambda r: f"{r[0]}-{r[1]}-{'f32' if r[2] else 'f64'}")
@pytest.mark.parametrize("bands", [1, 2, 37, None], ids=lambda b: f"B{b or 'auto'}")
@pytest.mark.parametrize("ring_set,mode", TABLES)
def test_bit_equal_to_reference(ext, monkeypatch, ring_set, mode, bands, rows):
    n, blocks, f32 = rows
    monkeypatch.setenv("ANOVOS_PIP_BLOCKS", str(blocks))
    table = edge_table(RING_SETS[ring_set], bands)
    B = len(table[1]) - 1
    pairs, refs = case(ring_set, n, B, f32)
    got, want = run(ext, pairs, table, bands=B, mode=mode), expected(pairs, refs)
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), f"{int((~same).sum())} elements differ"


def test_mixed_dtypes_and_lengths(ext):
    """An f32 pair of 1500 rows and an f64 pair of 70 rows in one call: one launch per dtype,
    each pair written to its own length."""
    rings = RING_SETS["overlap"]
    la, lo = points(rings, 1500, 2, seed=1)
    with np.errstate(over="ignore"):
        pairs = [(la.astype(np.float32), lo.astype(np.float32)), (la[:70], lo[:70])]
    refs = [reference(a, b, rings) for a, b in pairs]
    got, want = run(ext, pairs, edge_table(rings, 2)), expected(pairs, refs)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
