#!/usr/bin/env python3
"""What surface forces between ticks cost (SPEC.md 2e, sb_group_apply_surface_forces), beside the tick they sit in front of, a PARTICLE
impulse in the same run, and the route they replace.

Two bodies, each in a group of one device, `substeps` substeps per tick:
  cube   jelly_cube(n) with its surface triangles (tools/readback_bench.py surface_triangles): a volumetric body, few render particles
  cloth  a flat nx x nx sheet through mesh.from_triangle_mesh (springs and hinges): every particle is a render particle
Legs, ms per tick, EVERY LEG IN A FRESH GROUP of the same run (no leg inherits another's tables, graphs or tick state):
  (1) no call: the lazy tick boundary stays fused
  (2) one surface-force call before every tick (a weak wind: the body keeps its shape over the run)
  (3) one PARTICLE impulse before every tick: the same lost fusion with the smallest possible kernel behind it -- the comparison that
      matters, since the expected dominant cost of (2) is the lost fusion, not its two kernels
  (4) the route (2) replaces: get_positions + get_velocities + SPEC.md 2e vectorised in numpy + set_state before every tick, on the wall
      clock (its time is spent on the host and over PCIe), over fewer ticks
Legs 1 - 3 are timed with HIP events on the rank's stream (sb_profile_begin / sb_profile_end) and with the wall clock around the loop.
Beside them one call alone on a completed tick (event pair: launch overhead included) and snapshot_kernel the same way.
One JSON line; --out FILE also writes it there.

The KERNEL times come from a trace, in a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python3 tools/surface_force_bench.py --body cube --ticks 4 --skip-state-round-trip
  python3 tools/surface_force_bench.py --body cube --trace DIR/kt_kernel_trace.csv [--out FILE]
The second command needs no GPU. It reports the two kernels against this BYTES MODEL (m triangles, P render particles; what must cross
the memory system at least once, gathers counted once per distinct address), beside snapshot_kernel (24 B per particle) in the same trace:
  surface_force_triangle_kernel   12 m (corner indices) + 24 P (x and v of every render particle) + 16 m (J written)
  surface_force_vertex_kernel     36 P (particle index, offset, inverse mass, v read and written) + 12 m (incident lists) + 16 m (J read)

usage: surface_force_bench.py [--body cube|cloth] [--cube-n 256] [--cloth-n 256] [--substeps 20] [--ticks 20] [--repeats 3]
                              [--skip-state-round-trip] [--trace CSV] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM_TICKS = 3
FORCE = dict(wind=(0.02, 0.0, 0.01), normal=0.05, tangential=0.01, pressure=0.0)


def _stat(ms):
    return {"best": min(ms), "median": float(np.median(ms)), "all": [round(v, 5) for v in ms]}


def make_body(a):
    """-> (mesh, (m, 3) int32 render triangles over its particles, solver keywords)"""
    from softbodyunity_amd import from_triangle_mesh, jelly_cube
    if a.body == "cube":
        from readback_bench import surface_triangles
        return jelly_cube(a.cube_n), np.asarray(surface_triangles(a.cube_n), np.int32), {}
    nx = a.cloth_n
    u = np.arange(nx) * 0.05
    V = np.stack(np.meshgrid(u, [1.0], u, indexing="ij"), axis=-1).reshape(-1, 3)
    i = np.arange(nx - 1)
    q = (i[:, None] * nx + i[None, :]).ravel()
    T = np.concatenate([np.stack([q, q + nx, q + nx + 1], axis=1), np.stack([q, q + nx + 1, q + 1], axis=1)])
    mesh, particle_of_vertex = from_triangle_mesh(V, T)
    mesh.inv_mass[particle_of_vertex[[0, nx - 1]]] = 0.0
    return mesh, particle_of_vertex[T].astype(np.int32), dict(distance_compliance=1e-7, bending_compliance=1e-3, damping=0.05)


def model_bytes(m, parts, n):
    return {"surface_force_triangle_kernel": 12 * m + 24 * parts + 16 * m, "surface_force_vertex_kernel": 36 * parts + 12 * m + 16 * m, "snapshot_kernel": 24 * n}


def numpy_surface_forces(x, v, w, tri, wind, normal, tangential, pressure, dt):
    """SPEC.md 2e vectorised (float32 throughout; np.add.at sums in list order, not in ascending t per particle: the cost is what counts here)"""
    F = np.float32
    hn, ht, hp = (F(F(dt) * F(k)) / F(6) for k in (normal, tangential, pressure))
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    f = np.cross(x[b] - x[a], x[c] - x[a]).astype(np.float32)
    L2 = (f * f).sum(axis=1, dtype=np.float32)
    ok = (L2 >= F(2.0 ** -96)) & (L2 < np.inf)
    with np.errstate(all="ignore"):
        L = np.sqrt(L2)
        u = np.asarray(wind, np.float32) - (v[a] + v[b] + v[c]) / F(3)
        un = ((u * f).sum(axis=1, dtype=np.float32) / L2)[:, None] * f
        J = L[:, None] * (hn * un + ht * (u - un)) + hp * f
    J[~ok] = 0
    G = np.zeros_like(v)
    for k in (a, b, c):
        np.add.at(G, k, J)
    v += w[:, None] * G


def summarise_trace(path, m, parts, n):
    import csv
    us = {"surface_force_triangle_kernel": [], "surface_force_vertex_kernel": [], "snapshot_kernel": []}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in us:
                if k in r["Kernel_Name"]:
                    us[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    empty = [k for k, t in us.items() if not t]
    if empty:
        raise SystemExit(f"the trace holds no dispatch of {empty}")
    model = model_bytes(m, parts, n)
    return {"tool": "surface_force_bench --trace", "particles": n, "triangles": m, "render_particles": parts, "kernel_us": {k: _stat(t) for k, t in us.items()},
            "dispatches": {k: len(t) for k, t in us.items()}, "model_bytes": model,
            "model_gb_per_s": {k: model[k] / (float(np.median(us[k])) * 1e-6) / 1e9 for k in us}, "labels": "every dispatch of the run, warm-up included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default=None, help="summarise a rocprofv3 kernel trace of this tool instead of running (no GPU needed)")
    ap.add_argument("--body", choices=("cube", "cloth"), default="cube")
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--cloth-n", type=int, default=256)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-state-round-trip", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mesh, tri, kw = make_body(a)
    m, parts = int(tri.shape[0]), int(np.unique(tri).size)

    def emit(res):
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    if a.trace:
        return emit(summarise_trace(a.trace, m, parts, int(mesh.n)))
    from softbodyunity_amd import SoftbodyGroup, impulse_particles
    from embedding_bench import _clocks
    dt = 0.02
    free = int(np.nonzero(np.asarray(mesh.inv_mass) > 0)[0][mesh.n // 2])
    one_particle = impulse_particles([free], (0.0, 1e-7, 0.0))
    res = {"tool": "surface_force_bench", "body": a.body, "ticks": a.ticks, "repeats": a.repeats, "substeps": a.substeps, "particles": int(mesh.n), "triangles": m,
           "render_particles": parts, "force": FORCE,
           "timing": "ms per tick, every leg in a fresh group: HIP events on the rank's stream and wall clock around the loop (legs 1-3), wall clock (leg 4); per call (alone)",
           "clocks_before": _clocks()}
    calls = {"1_no_call": lambda g: None, "2_surface_forces": lambda g: g.apply_surface_forces(dt=dt, **FORCE), "3_one_particle_impulse": lambda g: g.apply_impulses(one_particle)}
    dev, wall, fused = {}, {}, {}
    for name, call in calls.items():
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps, **kw).Start()
        try:
            g.set_render_triangles(tri)
            r0 = g.rank(0)
            d0 = r0.stats()["device_bytes"]
            for _ in range(WARM_TICKS + 1):                  # first launches, the tables, the graph of either tick shape
                call(g); g.step()
            g.synchronize()
            dev[name], wall[name] = [], []
            for _ in range(a.repeats):
                f0 = r0.stats()["ticks_fused"]
                g.synchronize()
                t0 = time.perf_counter()
                r0.profile_begin()
                for _ in range(a.ticks):
                    call(g); g.step()
                dev[name].append(r0.profile_end() / a.ticks)
                g.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3 / a.ticks)
                fused[name] = r0.stats()["ticks_fused"] - f0
            if name == "2_surface_forces":
                res["table_bytes"] = r0.stats()["device_bytes"] - d0
                alone = {"surface_forces": [], "snapshot_kernel": []}
                for _ in range(a.repeats + 2):
                    g.step(); g.get_velocities()             # (completes the tick: no held-back kernel in the timed span)
                    r0.profile_begin(); call(g); alone["surface_forces"].append(r0.profile_end())
                    g.step(); g.get_velocities()
                    r0.profile_begin(); g.readback_begin(); alone["snapshot_kernel"].append(r0.profile_end())
                    g.readback_end()
                res["alone_device_ms"] = {k: _stat(t[2:]) for k, t in alone.items()}
            x = g.get_positions()
            res.setdefault("finite_at_the_end", {})[name] = bool(np.isfinite(x).all())
        finally:
            g.OnDestroy()
    res["legs_device_ms_per_tick"] = {k: _stat(t) for k, t in dev.items()}
    res["legs_wall_ms_per_tick"] = {k: _stat(t) for k, t in wall.items()}
    res["ticks_fused_per_leg"] = fused
    base = res["legs_device_ms_per_tick"]["1_no_call"]["median"]
    res["added_device_ms_per_tick"] = {k: res["legs_device_ms_per_tick"][k]["median"] - base for k in calls if k != "1_no_call"}
    res["model_bytes"] = model_bytes(m, parts, int(mesh.n))
    if not a.skip_state_round_trip:
        g = SoftbodyGroup(mesh, [0], substeps=a.substeps, **kw).Start()
        try:
            w = np.asarray(mesh.inv_mass, np.float32)
            x = np.zeros((mesh.n, 3), np.float32); v = np.zeros((mesh.n, 3), np.float32)
            ticks4 = max(2, a.ticks // 5)
            ms, partsum = [], []
            for rep in range(a.repeats + 1):
                g.synchronize()
                part = {"get_positions": 0.0, "get_velocities": 0.0, "numpy": 0.0, "set_state": 0.0}
                t0 = time.perf_counter()
                for t in range(ticks4):
                    ta = time.perf_counter(); g.get_positions(x)
                    tb = time.perf_counter(); g.get_velocities(v)
                    tc = time.perf_counter(); numpy_surface_forces(x, v, w, tri, dt=dt, **FORCE)
                    td = time.perf_counter(); g.set_state(x, v)
                    te = time.perf_counter()
                    for key, d in (("get_positions", tb - ta), ("get_velocities", tc - tb), ("numpy", td - tc), ("set_state", te - td)):
                        part[key] += d * 1e3 / ticks4
                    g.step()
                g.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / ticks4)
                partsum.append(part)
            res["4_replaced_route_wall_ms_per_tick"] = {"all": _stat(ms[1:]), "calls_ms": {k: float(np.median([p[k] for p in partsum[1:]])) for k in partsum[0]}, "ticks": ticks4}
        finally:
            g.OnDestroy()
    res["clocks_after"] = _clocks()
    emit(res)


if __name__ == "__main__":
    main()
