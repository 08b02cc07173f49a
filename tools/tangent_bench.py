#!/usr/bin/env python3
"""What render tangents (SPEC.md 6c, sb_set_render_uvs) cost per tick, beside the render-set readback with normals they ride on.

jelly_cube(n) with the render triangles of its surface, render-set-only, planar UVs (u, v = x, y of the rest pose over the cube's edge).
Three legs, each on a fresh solver, same process, same box, readbacks pipelined one tick behind as a renderer does:
  (a) no readback,  (b) readback with normals every tick,  (c) readback with normals and tangents every tick.
Timed with HIP events on the solver's stream (sb_profile_begin / sb_profile_end), legs interleaved and repeated, best and median of the
repeats reported, the box's clocks beside them; `tangents_ms_per_tick` is (c) - (b) of the medians. One JSON line; --out FILE also
writes it there.

usage: tangent_bench.py [--cube-n 256] [--ticks 40] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planar_uvs(mesh, n):
    """One UV per particle: the rest pose's x and y over the cube's edge."""
    rest = np.asarray(mesh.rest_pos, np.float64).reshape(-1, 3)
    return (rest[:, :2] / max(n - 1, 1)).astype(np.float32)


def _legs(mesh, tri, uv, substeps, ticks, repeats):
    from softbodyunity_amd import Softbody

    def piped(sb, n_ticks, tangents):
        for k in range(n_ticks):
            sb.step(); sb.readback_begin()
            if k:
                sb.readback_end(normals=True, tangents=tangents)
        sb.readback_end(normals=True, tangents=tangents)

    def plain(sb, n_ticks, tangents):
        for _ in range(n_ticks):
            sb.step()

    legs = {}
    solvers = {}
    try:
        for name in ("a_no_readback", "b_normals", "c_normals_tangents"):
            sb = Softbody(mesh, substeps=substeps).Start()
            solvers[name] = sb
            if name != "a_no_readback":
                sb.set_render_triangles(tri); sb.set_readback_render_set_only(True)
            if name == "c_normals_tangents":
                sb.set_render_uvs(uv)
            run = plain if name == "a_no_readback" else piped
            tangents = name == "c_normals_tangents"
            run(sb, 5, tangents); sb.synchronize()          # warm-up: first launches, buffers, the peek's tile subset
            legs[name] = (sb, run, tangents, [])
        for _ in range(repeats):                             # interleaved: a drift of the box's clocks lands on every leg alike
            for name, (sb, run, tangents, ms) in legs.items():
                sb.profile_begin()
                run(sb, ticks, tangents)
                ms.append(sb.profile_end() / ticks)
        out = {}
        for name, (sb, run, tangents, ms) in legs.items():
            st = sb.stats()
            out[name] = {"ms_per_tick_best": min(ms), "ms_per_tick_median": float(np.median(ms)), "ms_per_tick_all": [round(v, 5) for v in ms],
                         "readback_peek_tiles": st["readback_peek_tiles"], "t0_tiles": st["n_tiles"][0], "ticks_fused": st["ticks_fused"]}
        return out
    finally:
        for sb in solvers.values():
            sb.OnDestroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from softbodyunity_amd import jelly_cube
    from embedding_bench import _clocks
    from readback_bench import surface_triangles
    n = a.cube_n
    mesh = jelly_cube(n)
    tri = surface_triangles(n)
    res = {"tool": "tangent_bench", "ticks": a.ticks, "repeats": a.repeats, "timing": "HIP events on the solver's stream, per tick", "clocks_before": _clocks()}
    r = _legs(mesh, tri, planar_uvs(mesh, n), 20, a.ticks, a.repeats)
    r.update(particles=int(mesh.n), render_set_particles=int(np.unique(tri).size), render_triangles=int(tri.shape[0]), substeps=20,
             tangents_ms_per_tick=r["c_normals_tangents"]["ms_per_tick_median"] - r["b_normals"]["ms_per_tick_median"])
    res["cube"] = r
    res["clocks_after"] = _clocks()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
