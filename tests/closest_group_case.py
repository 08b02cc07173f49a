"""sb_group_readback_closest_points in a process of its own (tests/test_gpu_closest_points.py starts it, the way tests/test_gpu_raycast.py
starts tests/raycast_group_case.py): several ranks of one process on one device over the peer transport. Queries against the gathered
snapshot, the compact render set and an embedding, bit for bit the hits of tests/closest_ref.py on the oracle's positions (SPEC.md 6g); the
answer stays the snapshot's while another one is pending and a tick is issued; the hits feed sb_group_apply_impulses.
Prints `CLOSEST GROUP OK ...` or `CLOSEST GROUP MISMATCH ...`.

usage: closest_group_case.py <threads|walk> <ranks>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
import impulse_ref                                                     # noqa: E402
from closest_ref import HIT, bits, closest_ref, make_queries, same_hits   # noqa: E402
from embedding_ref import embedded_ref, lattice_cell_cages             # noqa: E402
from helpers import build_plan, make_oracle                            # noqa: E402
from readback_bench import surface_triangles                           # noqa: E402
from softbodyunity_amd import SoftbodyGroup, impulse_hits, native      # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402

FP = C.POINTER(C.c_float)
HP = C.POINTER(native.SbClosestHit)


def main(host, W):
    n, S, ticks, tile = 24, 6, 2, 64
    mesh = jelly_cube(n)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    rng = np.random.default_rng(41)
    why = []
    tri = surface_triangles(n)
    used = np.unique(tri)
    L = native.lib()
    Q = 37
    pts = rng.uniform(-4.0, n + 3.0, size=(Q, 3))
    q = make_queries(pts, np.where(np.arange(Q) % 3 == 1, rng.uniform(0.1, 3.0, size=Q), np.inf))
    q[[7, 19, 31], 3] = 1e-6                   # (the embedding's random triangles fill the cube: these limits lie below any distance there)
    m = 700
    cage = lattice_cell_cages(n, rng.integers(0, n - 1, size=(m, 3)), rng)
    w = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
    etri = rng.integers(0, m, size=(1500, 3)).astype(np.int32)
    g = SoftbodyGroup(mesh, [0] * W, substeps=S, tile_particles=tile, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", tuning=tune).Start()
    try:
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile))

        def raw(handle, r, count=None):
            r = np.ascontiguousarray(r, np.float32)
            hits = np.full(4 * max(len(r), 1), 0x7a7a7a7a, np.int32).view(HIT)
            rc = L.sb_group_readback_closest_points(handle, r.ctypes.data_as(FP), len(r) if count is None else count, hits.ctypes.data_as(HP))
            return rc, hits, bool((hits.view(np.int32) == 0x7a7a7a7a).all())
        if raw(None, q)[0] != native.SB_ERR_INVALID_ARG or raw(g._g, q, -1)[0] != native.SB_ERR_INVALID_ARG:
            why.append("null group or negative count accepted")
        rc, _, clean = raw(g._g, q)
        if rc != native.SB_ERR_STATE or not clean:
            why.append("a query before any readback has ended")
        g.readback_begin(); g.readback_end()
        rc, _, clean = raw(g._g, q)
        if rc != native.SB_ERR_STATE or not clean:
            why.append("a query on a snapshot without triangles")
        bad = q.copy(); bad[-1, 1] = np.nan

        def leg(name, source, tris):
            """ticks x (step, readback, query); with a second snapshot pending and a tick later the answer is the same"""
            for t in range(ticks):
                g.step(); o.step(0.02, S)
                g.readback_begin(); g.readback_end()
                want = closest_ref(source(o.x), tris, q)
                if not same_hits(g.closest_points(q), want):
                    why.append(f"leg {name}, tick {t}: group hits")
                if not ((want["triangle"] >= 0).any() and (want["triangle"] < 0).any()):
                    why.append(f"leg {name}, tick {t}: the queries all hit or all miss")
                rc, _, clean = raw(g._g, bad)
                if rc != native.SB_ERR_INVALID_ARG or not clean:
                    why.append(f"leg {name}: a NaN coordinate accepted")
            g.step(); o.step(0.02, S)
            moved = closest_ref(source(o.x), tris, q)
            g.readback_begin()
            g.step(); o.step(0.02, S)
            if not same_hits(g.closest_points(q), want):
                why.append(f"leg {name}: the answer changed with a snapshot pending and a tick issued")
            g.readback_end()
            if same_hits(moved, want) or not same_hits(g.closest_points(q), moved):
                why.append(f"leg {name}: the answer did not move on to the next snapshot")
            return moved
        g.set_render_triangles(tri)
        hits = leg("full", lambda x: x, tri)
        # the hits go back in as SURFACE impulses, in the whole mesh's numbering
        items = impulse_hits(hits, (0.0, -0.5, 0.25))
        g.apply_impulses(items)
        impulse_ref.apply(o.x, o.v, o.w, items, tri=tri)
        if not np.array_equal(bits(g.get_velocities()), bits(o.v)):
            why.append("velocities after the hits were applied as SURFACE impulses")
        g.readback_begin(); g.readback_end()
        full_hits = g.closest_points(q).copy()
        g.set_readback_render_set_only(True)
        g.readback_begin(); pos = g.readback_end()
        if not np.array_equal(bits(pos), bits(o.x[used])) or not same_hits(g.closest_points(q), full_hits):
            why.append("a full and a render-set snapshot of the same state give different hits")
        leg("render set", lambda x: x, tri)
        g.set_readback_render_set_only(False)
        g.set_render_triangles(np.zeros((0, 3), np.int32))
        rc, _, clean = raw(g._g, q)
        if rc != native.SB_ERR_STATE or not clean:
            why.append("a query after the triangles were set again")
        g.set_render_embedding(cage, w, etri)
        leg("embedding", lambda x: embedded_ref(x, cage, w), etri)
        after = [g.rank(r).stats() for r in range(W)]
        if sum(s["readback_peeks"] for s in after) == 0:
            why.append("no rank ever peeked")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append("final state")
    finally:
        g.OnDestroy()
    ok = not why
    print(("CLOSEST GROUP OK" if ok else "CLOSEST GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} ranks={W} render_set={used.size} render_vertices={m} queries={Q}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1], int(sys.argv[2])) else 1)
