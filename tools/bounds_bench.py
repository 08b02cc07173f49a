#!/usr/bin/env python3
"""What the bounding box (SPEC.md 6d, sb_set_readback_bounds / sb_get_bounds) costs, beside the readback it rides on.

jelly_cube(n) with the render triangles of its surface, ONE solver, same process, same box. Per mode -- full snapshots (n rows reduced) and
render-set-only (the surface particles) -- readbacks with normals every tick, pipelined one tick behind as a renderer does:
  (1) bounds off,  (2) bounds on,
interleaved and repeated (the setting is a switch: no second solver), timed with HIP events on the solver's stream (sb_profile_begin /
sb_profile_end), best and median of the repeats; `bounds_ms_per_readback` is (2) - (1) of the medians. Beside it, in full mode, the time of
snapshot_kernel alone -- it moves the same bytes, the natural floor of a reduction over the snapshot -- as the HIP-event time of one
sb_readback_begin on a completed tick (the snapshot kernel is all that call puts on the solver's stream then).
  (3) sb_get_bounds against sb_get_positions on a completed tick: wall clock of the blocking call, and the HIP-event time of the query.
One JSON line; --out FILE also writes it there.

usage: bounds_bench.py [--cube-n 256] [--ticks 20] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _piped(sb, n_ticks, bounds):
    for k in range(n_ticks):
        sb.step(); sb.readback_begin()
        if k:
            sb.readback_end(normals=True, bounds=bounds)
    return sb.readback_end(normals=True, bounds=bounds)


def _stat(ms):
    return {"best": min(ms), "median": float(np.median(ms)), "all": [round(v, 5) for v in ms]}


def _mode(sb, compact, ticks, repeats):
    sb.set_readback_render_set_only(compact)
    legs = {"1_normals": [], "2_normals_bounds": []}
    for name in legs:                                        # warm-up: first launches, buffers, the peek's tile subset
        sb.set_readback_bounds(name == "2_normals_bounds")
        _piped(sb, 3, name == "2_normals_bounds"); sb.synchronize()
    box = None
    for _ in range(repeats):                                 # interleaved: a drift of the box's clocks lands on both legs alike
        for name, ms in legs.items():
            on = name == "2_normals_bounds"
            sb.set_readback_bounds(on)
            sb.profile_begin()
            got = _piped(sb, ticks, on)
            ms.append(sb.profile_end() / ticks)
            if on:
                box = got[-1]
    out = {name: _stat(ms) for name, ms in legs.items()}
    out["bounds_ms_per_readback"] = out["2_normals_bounds"]["median"] - out["1_normals"]["median"]
    out["rows_reduced"] = int(len(sb.render_set())) if compact else int(sb.n)
    out["box"] = [[float(v) for v in box[0]], [float(v) for v in box[1]]]
    return out


def _snapshot_kernel(sb, repeats):
    """HIP-event time of sb_readback_begin's work on the solver's stream in full mode on a completed tick: snapshot_kernel"""
    sb.set_readback_render_set_only(False); sb.set_readback_bounds(False)
    ms = []
    for _ in range(repeats + 1):
        sb.step(); sb.get_velocities()                       # (completes the tick: no peek, no held-back kernel in the timed span)
        sb.profile_begin()
        sb.readback_begin()
        ms.append(sb.profile_end())
        sb.readback_end()
    return _stat(ms[1:])


def _query(sb, repeats):
    wall = {"sb_get_bounds": [], "sb_get_positions": []}
    dev = []
    out = np.zeros((sb.n, 3), np.float32)
    for _ in range(repeats + 1):
        for name in wall:
            sb.step(); sb.synchronize()
            t0 = time.perf_counter()
            if name == "sb_get_bounds":
                sb.get_bounds()
            else:
                sb.get_positions(out)
            wall[name].append((time.perf_counter() - t0) * 1e3)
        sb.step(); sb.synchronize()
        sb.profile_begin(); sb.get_bounds(); dev.append(sb.profile_end())
    return {"wall_ms": {k: _stat(v[1:]) for k, v in wall.items()}, "sb_get_bounds_device_ms": _stat(dev[1:]),
            "bytes_to_host": {"sb_get_bounds": 32, "sb_get_positions": int(sb.n) * 12}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube-n", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from softbodyunity_amd import Softbody, jelly_cube
    from embedding_bench import _clocks
    from readback_bench import surface_triangles
    n = a.cube_n
    mesh = jelly_cube(n)
    tri = surface_triangles(n)
    res = {"tool": "bounds_bench", "ticks": a.ticks, "repeats": a.repeats, "substeps": 20, "particles": int(mesh.n),
           "timing": "HIP events on the solver's stream, per tick (legs 1, 2); per call (snapshot_kernel, leg 3)", "clocks_before": _clocks()}
    sb = Softbody(mesh, substeps=20).Start()
    try:
        sb.set_render_triangles(tri)
        res["full"] = _mode(sb, False, a.ticks, a.repeats)
        res["full"]["snapshot_kernel_ms"] = _snapshot_kernel(sb, a.repeats)
        res["render_set"] = _mode(sb, True, a.ticks, a.repeats)
        sb.set_readback_render_set_only(False)
        res["query"] = _query(sb, a.repeats)
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
