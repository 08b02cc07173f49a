#!/usr/bin/env python3
"""What sb_readback_begin + sb_readback_end cost the HOST, per render mode: wall clock around pipelined calls (one readback in flight while
the next begins) on jelly_cube(8), where the kernels and copies are next to nothing and the call overhead is what is left. For A/B runs of
plugin variants (SB_LIB_VARIANT, one process per run, alternating). One JSON line: microseconds per begin + end pair, median and best of
the repeats.

usage: readback_host_bench.py [--calls 1000] [--repeats 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    from embedding_ref import lattice_cell_cages
    from readback_bench import surface_triangles
    from softbodyunity_amd import Softbody, jelly_cube
    n = 8
    mesh = jelly_cube(n)
    rng = np.random.default_rng(5)
    m = 600
    cage = lattice_cell_cages(n, rng.integers(0, n - 1, size=(m, 3)), rng)
    w = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
    etri = rng.integers(0, m, size=(1200, 3)).astype(np.int32)
    sb = Softbody(mesh, substeps=4).Start()
    res = {"tool": "readback_host_bench", "variant": os.environ.get("SB_LIB_VARIANT", "") or "product", "calls": a.calls, "repeats": a.repeats, "us_per_begin_end": {}}

    def piped(calls):
        sb.readback_begin()
        for _ in range(calls - 1):
            sb.readback_begin(); sb.readback_end()
        sb.readback_end()

    def leg(name):
        sb.step(); piped(50); sb.synchronize()
        us = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            piped(a.calls)
            us.append(1e6 * (time.perf_counter() - t0) / a.calls)
        res["us_per_begin_end"][name] = {"median": round(float(np.median(us)), 3), "best": round(min(us), 3)}

    try:
        leg("full")
        sb.set_render_triangles(surface_triangles(n)); leg("normals")
        sb.set_readback_render_set_only(True); leg("render_set_normals")
        sb.set_render_uvs(rng.uniform(0, 1, size=(mesh.n, 2)).astype(np.float32)); leg("render_set_normals_tangents")
        sb.set_readback_bounds(True); leg("render_set_normals_tangents_bounds")
        sb.set_render_triangles(np.zeros((0, 3), np.int32))
        sb.set_render_embedding(cage, w, etri); leg("embedded_normals_bounds")
        sb.set_render_uvs(rng.uniform(0, 1, size=(m, 2)).astype(np.float32)); leg("embedded_normals_tangents_bounds")
    finally:
        sb.OnDestroy()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
