#!/usr/bin/env python3
"""What a closest-point query against the deformed render mesh costs (SPEC.md 6g, sb_group_readback_closest_points).

jelly_cube(n) with the render triangles of its surface in render-set mode (256^3: 390 k vertices, 780 k triangles), a group of ONE device, a
snapshot that has ended and nothing in flight. Wall clock of the blocking call -- upload, two launches per batch of 256, download, one
stream synchronisation each: what the caller waits for --, median and best of --calls calls, for 1, 64 and 1 024 queries scattered inside and
around the body. Beside it, in the same process on the same snapshot:
  * sb_group_readback_raycast with as many rays: the twin, same launch shape, same buffers;
  * sb_group_get_bounds on a completed tick: the existing synchronous query of the same kind, the floor of a one-query call;
  * the replaced route: the numpy reference of SPEC.md 6g (tests/closest_ref.py: float32, vectorised over the triangles, one thread) over
    the pinned snapshot, per query, over --cpu-queries queries, and whether it names the GPU's hits bit for bit.
The kernels' own durations are not in here: they come from a `rocprofv3 --kernel-trace` run of this script (no counters in that run);
--trace-summary DIR reads the *_kernel_trace.csv such a run left under DIR and writes the per-kernel figures to --out instead.
One JSON line; --out FILE also writes it there.

usage: closest_point_bench.py [--cube-n 256] [--calls 200] [--cpu-queries 5] [--out FILE]
       closest_point_bench.py --trace-summary DIR --out FILE
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32 = np.float32


def _stat(ms):
    return {"median": float(np.median(ms)), "best": float(min(ms)), "calls": len(ms)}


def _queries(n, count, rng):
    """points inside and within a quarter of the cube's size around it; every fourth limited to a few lattice spacings"""
    q = np.zeros((count, 4), F32)
    q[:, 0:3] = rng.uniform(-0.25 * n, 1.25 * n, size=(count, 3))
    q[:, 3] = np.where(np.arange(count) % 4 == 3, rng.uniform(0.5, 8.0, size=count), np.inf)
    return q


def _timed(fn, calls):
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stat(ms)


def _write(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def trace_summary(folder, out):
    """per kernel of the query and of the ray cast: calls, median / best / total duration in microseconds, from rocprofv3's kernel trace"""
    rows = {}
    files = [os.path.join(d, f) for d, _, fs in os.walk(folder) for f in fs if f.endswith("kernel_trace.csv")]
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].split("(")[0].split()[-1]
                if any(k in name for k in ("closest_", "raycast_", "bounds_")):       # (a launch's shape tells the batches of 1, 64 and 256 apart)
                    key = f'{name} grid {r.get("Grid_Size_X", "?")}x{r.get("Grid_Size_Y", "?")} vgprs {r.get("VGPR_Count", "?")}'
                    rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = {"tool": "closest_point_bench --trace-summary", "source": "rocprofv3 --kernel-trace, no counters", "files": len(files), "unit": "us",
           "kernels": {k: {"calls": len(v), "median": float(np.median(v)), "best": float(min(v)), "worst": float(max(v)), "total": float(sum(v))} for k, v in sorted(rows.items())}}
    _write(res, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cpu-queries", type=int, default=5)
    ap.add_argument("--trace-summary", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary, a.out)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from closest_ref import closest_ref, same_hits
    from embedding_bench import _clocks
    from raycast_bench import _rays
    from readback_bench import surface_triangles
    from softbodyunity_amd import SoftbodyGroup, jelly_cube
    n = a.cube_n
    mesh = jelly_cube(n)
    tri = surface_triangles(n)
    rng = np.random.default_rng(9)
    res = {"tool": "closest_point_bench", "particles": int(mesh.n), "triangles": int(len(tri)), "substeps": 20,
           "timing": "wall clock of the blocking call, ms", "clocks_before": _clocks()}
    g = SoftbodyGroup(mesh, [0], substeps=20).Start()
    try:
        g.set_render_triangles(tri); g.set_readback_render_set_only(True)
        for _ in range(3):
            g.step()
        g.readback_begin()
        pos = g.readback_end()
        ids = g.render_set()
        res["render_set"] = int(len(ids))
        g.synchronize()
        res["closest_points_wall_ms"], res["raycast_wall_ms"] = {}, {}
        for count in (1, 64, 1024):
            q = _queries(n, count, rng)
            hits = g.closest_points(q)                         # (the first call allocates)
            res["closest_points_wall_ms"][str(count)] = dict(_timed(lambda: g.closest_points(q), a.calls), queries_hit=int((hits["triangle"] >= 0).sum()))
            rays = _rays(n, count, rng)
            rhits = g.raycast(rays)
            res["raycast_wall_ms"][str(count)] = dict(_timed(lambda: g.raycast(rays), a.calls), rays_hit=int((rhits["triangle"] >= 0).sum()))
        res["sb_group_get_bounds_wall_ms"] = _timed(g.get_bounds, a.calls)
        # the replaced route: the host's walk over the pinned snapshot (compact rows: translate the triangles once, as a component does)
        compact_of = np.zeros(mesh.n, np.int64); compact_of[ids] = np.arange(len(ids))
        ctri = compact_of[tri].astype(np.int32)
        q = _queries(n, max(a.cpu_queries, 1), rng)
        gpu = g.closest_points(q)
        ms, same = [], 0
        for r in range(a.cpu_queries):
            t0 = time.perf_counter()
            want = closest_ref(np.asarray(pos, F32), ctri, q[r:r + 1])       # (the vertices move every tick: the gather is part of every walk)
            ms.append((time.perf_counter() - t0) * 1e3)
            same += int(same_hits(want, gpu[r:r + 1]))
        if ms:
            res["numpy_reference_one_thread_ms_per_query"] = dict(_stat(ms), same_bits_as_gpu=f"{same} of {a.cpu_queries}",
                                                                  how="tests/closest_ref.py closest_ref: numpy float32, vectorised over the triangles, one thread")
    finally:
        g.OnDestroy()
    res["clocks_after"] = _clocks()
    _write(res, a.out)


if __name__ == "__main__":
    main()
