#!/usr/bin/env python3
"""What a ray cast against the deformed render mesh costs (SPEC.md 6e, sb_readback_raycast).

jelly_cube(n) with the render triangles of its surface in render-set mode (256^3: 390 k vertices, 780 k triangles), ONE solver, a snapshot
that has ended and nothing in flight. Wall clock of the blocking call, median and best of --calls calls, for 1, 64 and 1 024 rays aimed at
the body from outside. Beside it, in the same process:
  * sb_get_bounds on a completed tick: the existing synchronous query of the same kind (two small kernels, a few bytes to the host, one
    stream synchronisation), the floor of a one-ray call;
  * the brute-force walk of the same triangles over the pinned snapshot on ONE CPU thread -- what a host does today: numpy float32,
    vectorised over the triangles (no Python per triangle), the same Moeller-Trumbore statements -- per ray, over --cpu-rays rays.
One JSON line; --out FILE also writes it there.

usage: raycast_bench.py [--cube-n 256] [--calls 200] [--cpu-rays 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32 = np.float32


def _stat(ms):
    return {"median": float(np.median(ms)), "best": float(min(ms)), "calls": len(ms)}


def _rays(n, count, rng):
    """from a sphere around the cube towards points of it; every sixth past it"""
    o = rng.normal(size=(count, 3)); o = (n - 1) / 2 + 2.0 * n * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(0.0, n - 1.0, size=(count, 3))
    target[::6] += 4.0 * n
    d = target - o
    rays = np.zeros((count, 8), F32)
    rays[:, 0:3] = o; rays[:, 3] = np.inf; rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return rays


def _cpu_walk(pa, e1, e2, ray):
    """one ray against every triangle: (triangle, t) of the nearest hit"""
    o, d = ray[0:3], ray[4:7]
    with np.errstate(all="ignore"):
        P = np.cross(d[None, :], e2)
        det = np.einsum("ij,ij->i", e1, P)
        inv = F32(1) / det
        T = o[None, :] - pa
        u = np.einsum("ij,ij->i", T, P) * inv
        Q = np.cross(T, e1)
        v = np.einsum("ij,ij->i", Q, d[None, :].repeat(len(Q), 0)) * inv
        t = np.einsum("ij,ij->i", e2, Q) * inv
        ok = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= ray[3])
    if not ok.any():
        return -1, 0.0
    k = int(np.argmin(np.where(ok, t, np.inf)))
    return k, float(t[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cpu-rays", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from softbodyunity_amd import Softbody, jelly_cube
    from embedding_bench import _clocks
    from readback_bench import surface_triangles
    n = a.cube_n
    mesh = jelly_cube(n)
    tri = surface_triangles(n)
    rng = np.random.default_rng(8)
    res = {"tool": "raycast_bench", "particles": int(mesh.n), "triangles": int(len(tri)), "substeps": 20,
           "timing": "wall clock of the blocking call, ms", "clocks_before": _clocks()}
    sb = Softbody(mesh, substeps=20).Start()
    try:
        sb.set_render_triangles(tri); sb.set_readback_render_set_only(True)
        for _ in range(3):
            sb.step()
        sb.readback_begin()
        pos = sb.readback_end()
        ids = sb.render_set()
        res["render_set"] = int(len(ids))
        sb.synchronize()
        res["raycast_wall_ms"] = {}
        for count in (1, 64, 1024):
            rays = _rays(n, count, rng)
            hits = sb.raycast(rays)                           # (the first call allocates)
            ms = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                sb.raycast(rays)
                ms.append((time.perf_counter() - t0) * 1e3)
            res["raycast_wall_ms"][str(count)] = dict(_stat(ms), rays_hit=int((hits["triangle"] >= 0).sum()))
        ms = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            sb.get_bounds()
            ms.append((time.perf_counter() - t0) * 1e3)
        res["sb_get_bounds_wall_ms"] = _stat(ms)
        # the host's walk over the pinned snapshot (compact rows: translate the triangles once, as a component does)
        compact_of = np.zeros(mesh.n, np.int64); compact_of[ids] = np.arange(len(ids))
        ctri = compact_of[tri]
        rays = _rays(n, a.cpu_rays, rng)
        gpu = sb.raycast(rays)
        ms, agree = [], 0
        for r in range(a.cpu_rays):
            t0 = time.perf_counter()
            p = np.asarray(pos, F32)
            pa = p[ctri[:, 0]]; e1 = p[ctri[:, 1]] - pa; e2 = p[ctri[:, 2]] - pa       # (the vertices move every tick: part of every walk)
            k, t = _cpu_walk(pa, e1, e2, rays[r])
            ms.append((time.perf_counter() - t0) * 1e3)
            agree += int(k == gpu[r]["triangle"])
        res["cpu_walk_one_thread_ms_per_ray"] = dict(_stat(ms), same_triangle_as_gpu=f"{agree} of {a.cpu_rays}",
                                                     how="numpy float32, vectorised over the triangles, one thread")
    finally:
        sb.OnDestroy()
    res["clocks_after"] = _clocks()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
