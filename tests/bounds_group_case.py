"""sb_group_set_readback_bounds / sb_group_readback_get_bounds / sb_group_get_bounds in a process of its own (tests/test_gpu_bounds.py starts
it, the way tests/test_gpu_render_tangents.py starts tests/tangent_group_case.py): two ranks of one process on one device over the peer
transport. The readback box in all three modes -- the gathered snapshot, the compact render set, an embedding whose cages straddle the rank
boundary -- and the query that combines the ranks' own boxes on the host, bit for bit tests/bounds_ref.py on the oracle's positions (SPEC.md 6d).
Prints `BOUNDS GROUP OK ...` or `BOUNDS GROUP MISMATCH ...`.

usage: bounds_group_case.py <threads|walk>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import oracle                                              # noqa: E402  (test infrastructure: the checker)
from bounds_ref import bits, bounds_ref, merge, same_box               # noqa: E402
from embedding_ref import embedded_ref, lattice_cell_cages             # noqa: E402
from helpers import build_plan, make_oracle                            # noqa: E402
from readback_bench import surface_triangles                           # noqa: E402
from softbodyunity_amd import SoftbodyGroup, native                    # noqa: E402
from softbodyunity_amd.mesh import jelly_cube                          # noqa: E402

FP = C.POINTER(C.c_float)


def main(host):
    n, S, ticks, tile = 24, 6, 2, 64
    mesh = jelly_cube(n)
    tune = native.SbTuning(); native.lib().sb_tuning_default(C.byref(tune)); tune.peek_min_tiles = 0       # small launches peek too
    rng = np.random.default_rng(31)
    why = []
    tri = surface_triangles(n)
    used = np.unique(tri)
    L = native.lib()
    g = SoftbodyGroup(mesh, [0, 0], substeps=S, tile_particles=tile, halo_transport=native.SB_TRANSPORT_PEER, walk=host == "walk", tuning=tune).Start()
    try:
        r0 = g.rank(0); r0.n = mesh.n            # (24^3 under the automatic partition: every rank numbers the whole mesh)
        owner = r0.owner()
        grid = owner.reshape(n, n, n)
        lo, hi = grid[:-1, :-1, :-1].copy(), grid[:-1, :-1, :-1].copy()
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c = grid[dz:n - 1 + dz, dy:n - 1 + dy, dx:n - 1 + dx]
                    lo = np.minimum(lo, c); hi = np.maximum(hi, c)
        straddle = np.argwhere(lo != hi)[:, ::-1]      # (z, y, x) -> (x, y, z)
        interior = np.argwhere(lo == hi)[:, ::-1]
        if len(straddle) == 0:
            why.append("no cell straddles the rank boundary")
        cells = np.concatenate([straddle[rng.integers(0, max(len(straddle), 1), 350)], interior[rng.integers(0, len(interior), 350)]])
        cage = lattice_cell_cages(n, cells, rng)
        m = cage.shape[0]
        w = rng.uniform(-0.5, 1.5, size=(m, 4)).astype(np.float32)
        o = make_oracle(oracle, mesh, build_plan(mesh, tile_particles=tile))
        buf = np.zeros(3, np.float32)
        p = buf.ctypes.data_as(FP)

        def status(fn, *a):
            return fn(*a)
        # the contract holds on a group as well
        if status(L.sb_group_set_readback_bounds, None, 1) != native.SB_ERR_INVALID_ARG or status(L.sb_group_get_bounds, None, p, p) != native.SB_ERR_INVALID_ARG:
            why.append("null group accepted")
        if status(L.sb_group_readback_get_bounds, g._g, None, p) != native.SB_ERR_INVALID_ARG or status(L.sb_group_get_bounds, g._g, p, None) != native.SB_ERR_INVALID_ARG:
            why.append("null array accepted")
        if status(L.sb_group_readback_get_bounds, g._g, p, p) != native.SB_ERR_STATE:
            why.append("a box before any readback has ended")
        g.readback_begin(); g.readback_end()
        g.set_readback_bounds(True)
        if status(L.sb_group_readback_get_bounds, g._g, p, p) != native.SB_ERR_STATE:
            why.append("a box for a snapshot begun with bounds off")

        def leg(name, delivered):
            """ticks x (step, readback with bounds, query between the ticks)"""
            for t in range(ticks):
                g.step(); o.step(0.02, S)
                g.readback_begin()
                if status(L.sb_group_set_readback_bounds, g._g, 0) != native.SB_ERR_STATE:
                    why.append(f"leg {name}: the setting changed while a readback was pending")
                got = g.readback_end(bounds=True)
                pos, box = got[0], got[-1]
                want = delivered(o.x)
                if not np.array_equal(bits(pos), bits(want)):
                    why.append(f"leg {name}, tick {t}: positions")
                if not same_box(box, bounds_ref(want)):
                    why.append(f"leg {name}, tick {t}: readback box {box} for {bounds_ref(want)}")
                q = g.get_bounds()
                if not same_box(q, bounds_ref(o.x)):
                    why.append(f"leg {name}, tick {t}: sb_group_get_bounds {q} for {bounds_ref(o.x)}")
        leg("full", lambda x: x)
        # ... which is the min / max of what the ranks own
        if not same_box(merge([bounds_ref(o.x[owner == r]) for r in (0, 1)]), bounds_ref(o.x)) or not (0 < (owner == 0).sum() < mesh.n):
            why.append("the ranks' boxes do not combine to the whole body's")
        g.set_render_triangles(tri); g.set_readback_render_set_only(True)
        leg("render set", lambda x: x[used])
        g.set_readback_render_set_only(False)
        g.set_render_triangles(np.zeros((0, 3), np.int32))
        g.set_render_embedding(cage, w)
        leg("embedding", lambda x: embedded_ref(x, cage, w))
        peeks = sum(g.rank(r).stats()["readback_peeks"] for r in (0, 1))
        if peeks == 0:
            why.append("no rank ever peeked")
        if not (np.array_equal(bits(g.get_positions()), bits(o.x)) and np.array_equal(bits(g.get_velocities()), bits(o.v))):
            why.append("final state")
    finally:
        g.OnDestroy()
    ok = not why
    print(("BOUNDS GROUP OK" if ok else "BOUNDS GROUP MISMATCH " + "; ".join(why[:12])), f"host={host} render_set={used.size} render_vertices={m}")
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(sys.argv[1]) else 1)
