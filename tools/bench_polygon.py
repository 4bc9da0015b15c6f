"""Time point-in-polygon membership (K33) and sweep its band count.

Workload: --rows seeded points scattered uniformly over 1.5 x the bounding
box of a mildly jittered E-gon (E from --edges), lat / lon as f64 columns
(and f32 for the kernel table).

  (a) sweep: the binding alone (table upload, image kernel, membership
      kernel; device events) for every B of --bands and both table
      placements where the image fits LDS, next to the same call on 1 024
      rows, which is the part that does not depend on the rows. Bytes are the
      two-column read plus the f32 write.
  (b) location_in_polygon end to end (wall clock around a synchronised call,
      peak of allocated memory beyond the frame), alternated with the
      whole-column torch expression it replaces (geo_utils.point_in_polygons
      on all rows x all edges) on the first --old-elems / E rows.
  (c) agreement of the two on those rows.

    python tools/bench_polygon.py --rows 16000000 --edges 4 100 2000 20000
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def polygon(E: int, seed: int):
    rng = np.random.default_rng(seed + E)
    a = (np.arange(E) + 0.8 * rng.random(E)) * (2 * np.pi / E)
    r = 1 + 0.1 * rng.random(E) * min(1.0, 40.0 / E)
    return np.column_stack([10 + 6 * r * np.cos(a), 50 + 4 * r * np.sin(a)]).tolist()


def events_ms(fn, warmup: int, reps: int):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms)


def wall_peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t) * 1e3, torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--edges", type=int, nargs="*", default=[4, 100, 2000, 20000])
    ap.add_argument("--bands", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024, 4096])
    ap.add_argument("--old-elems", type=float, default=1.6e9, help="rows x edges the old expression is run on")
    ap.add_argument("--max-list", type=int, default=600, help="skip band counts with longer mean lists")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_polygon needs a GPU: a CPU timing says nothing about the kernel")
    from anovos_amd.core.frame import AnovosFrame, Column
    from anovos_amd.data_transformer import geo_utils as gu
    from anovos_amd.data_transformer import geospatial as geo
    from anovos_amd.ops import backend
    from anovos_amd.ops.polygon import edge_table

    ext = backend.require_hip()
    n = args.rows
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    lat = 50 + 1.5 * 8.8 * (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) - 0.5)
    lon = 10 + 1.5 * 13.2 * (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) - 0.5)
    cols = {"f64": (lat, lon), "f32": (lat.float(), lon.float())}
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    idf = AnovosFrame({"lat": Column("lat", "double", lat), "lon": Column("lon", "double", lon)}, "cuda")

    for E in args.edges:
        ring = polygon(E, args.seed)
        auto = len(edge_table([ring])[1]) - 1
        for B in sorted(set(args.bands + [auto])):
            table = [torch.from_numpy(t) for t in edge_table([ring], B)]
            if len(table[2]) / B > args.max_list:
                continue  # minutes per call: not a candidate
            nbytes = ext.PIP_RECORD_BYTES * len(table[2]) + 4 * (B + 4)
            for place in ["lds", "global"] if nbytes <= ext.PIP_LDS_BYTES else ["global"]:
                row = {"sweep": E, "bands": B, "auto": B == auto, "records": len(table[2]), "table": place}
                for dt, (la, lo) in cols.items():
                    call = lambda m: ext.points_in_polygons([la[:m]], [lo[:m]], *table, [out[:m]], bands=B, table=place)
                    ms = events_ms(lambda: call(n), args.warmup, args.reps)
                    ms0 = events_ms(lambda: call(1024), args.warmup, args.reps)
                    traffic = n * (2 * la.element_size() + 4)
                    row[dt] = {"call_ms": round(ms, 3), "call_1024_rows_ms": round(ms0, 3),
                               "TB_per_s_of_call": round(traffic / ms / 1e9, 3)}
                print(json.dumps(row), flush=True)

        m = int(min(n, args.old_elems // E))
        old_cols = lat[:m], lon[:m]

        def old():
            inside = gu.point_in_polygons(*old_cols, [ring]).to(torch.float32)
            return torch.where(torch.isnan(old_cols[0]) | torch.isnan(old_cols[1]), torch.full_like(inside, float("nan")), inside)

        new = lambda: geo.location_in_polygon(idf, ["lat"], ["lon"], [ring]).col("lat_lon_in_polygon").data
        new(), old()
        new_ms, old_ms = [], []
        for _ in range(args.reps):
            got, ms, peak = wall_peak(new)
            new_ms.append(ms)
            want, ms, old_peak = wall_peak(old)
            old_ms.append(ms)
        print(json.dumps({"end_to_end": E, "rows": n, "new_ms": round(statistics.median(new_ms), 3), "new_peak_bytes": peak,
                          "old_rows": m, "old_ms": round(statistics.median(old_ms), 3), "old_peak_bytes": old_peak,
                          "per_row_speedup": round(statistics.median(old_ms) / m / (statistics.median(new_ms) / n), 1),
                          "equal_on_old_rows": bool(torch.equal(got[:m], want)),
                          "inside_fraction": round(float(got.mean()), 4)}), flush=True)
        del got, want


if __name__ == "__main__":
    main()
